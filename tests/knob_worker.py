"""Worker process of tests/test_knob_forms_gpu.py: a fixed list of scenes from fixed seeds, run with whatever IAGO_*
environment its parent gave it, written as one .npz.  Several tuning knobs are latched in a `static` of the library on
first use (IAGO_VALUE_TINY, IAGO_VALUE_PERSIST, IAGO_POLICY_GRID, IAGO_PERSISTENT_PAIR, IAGO_PERSISTENT_POLICY_XCDS),
so a form that only such a knob selects needs a process of its own.

    python tests/knob_worker.py <out.npz>

Scenes (the smallest shapes at which each form can still go wrong; every float32 saved as its bits):
  vd_<count>   Value net, shipped weights, device-counted through a gather list (a permutation) over a bound of
               VALUE_BOUND boards, out prefilled with NaN: rows past the count must stay NaN, rows inside it be written
  vh_<n>       Value net, host-counted, the first n boards
  ph_<parts>_<n>, pd_<parts>_<count>
               SLPolicy, shipped weights, forward_boards_split3 host-counted on n boards / device-counted (the first
               `count` rows of a gather list over POLICY_BOUND boards), as `parts` launches
  s<G>_*       one persistent search of G games, SEARCH_SIMS[0] then SEARCH_SIMS[1] playouts with subtree reuse: node
               records (visit counts, Q, P, actions, child ranges; dead records zeroed), roots, stored values, leaf
               values, moves, visit counts of the moves, the recorded rollout results, error words
  sched_*      diagnostics that depend on the schedule (not compared): pairs of boards walked together
  env          the IAGO_* variables this process saw
"""
import json
import os
import sys
import time
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")

VALUE_BOUND = 600
VALUE_DEV_COUNTS = (0, 1, 3, 4, 255, 256, 257, 511, 512, 513, 600)
VALUE_HOST_ROWS = (1, 2, 3, 4, 5, 256, 257, 512, 513, 600)
POLICY_HOST_ROWS = (1, 5, 7, 64)
POLICY_BOUND, POLICY_DEV_COUNTS = 7, (0, 1, 6)
POLICY_PARTS = (1, 2)
SEARCH_GAMES = (20, 96)          # (20: the oracle-checked size, 8 net workgroups; 96: a backlog for the pair walk)
SEARCH_SIMS = (100, 45)
SEARCH_IDLE = 5                  # a game that takes no part


def value_positions():
    """Rows 0..255: the traced positions of tests/golden/nets_shipped.npz (their float64 outputs are committed); the
    others: tests.gpu_util.random_positions(seed=77), the source of test_conv_gpu.py's counted test."""
    from tests.gpu_util import random_positions
    gold = np.load(os.path.join(GOLDEN, "nets_shipped.npz"))
    own, opp = random_positions(VALUE_BOUND - 256, seed=77)
    return np.concatenate([gold["own"], own]), np.concatenate([gold["opp"], opp])


def value_perm():
    import torch
    return torch.randperm(VALUE_BOUND, generator=torch.Generator().manual_seed(600))


def policy_perm():
    import torch
    return torch.randperm(POLICY_BOUND, generator=torch.Generator().manual_seed(7))


def search_positions(G):
    from tests.gpu_util import random_positions
    own, opp = random_positions(G, seed=78)
    own[: G // 2] = 0x0000000810000000
    opp[: G // 2] = 0x0000001008000000
    return own, opp


def search_engine(G, nets):
    """The engine of the search scene (the parent builds the same one for the oracle's probe)."""
    engine, ops, policy, value, rw = nets
    return engine.BatchedMCTS(G, policy, value, rw, lmbda=0.5, c_puct=1.0, n_thr=15,
                              capacity=engine.suggest_capacity(sum(SEARCH_SIMS), 15, moves=2), seed=21, game_id_base=300,
                              z_log_rows=max(SEARCH_SIMS), persistent=True, net_workgroups=8 if G == 20 else None)


def shipped_nets():
    import torch
    from iago_amd import engine, network, ops
    assert torch.cuda.is_available()
    policy = network.SLPolicy().load_npz(os.path.join(GOLDEN, "sl_model.npz")).cuda().eval()
    value = network.Value().load_npz(os.path.join(GOLDEN, "value_model.npz")).cuda().eval()
    with open(os.path.join(GOLDEN, "simulate.json")) as f:
        g = json.load(f)
    return engine, ops, policy, value, ops.RolloutWeights(g["shipped_w"], g["shipped_b"])


def bits(t):
    return t.detach().contiguous().cpu().numpy().view(np.uint32).copy()


def value_scenes(out, nets):
    import torch
    engine, ops, policy, value, rw = nets
    own, opp = value_positions()
    o, p = ops.bits_to_tensor(own), ops.bits_to_tensor(opp)
    perm = value_perm().cuda()
    with torch.no_grad():
        for count in VALUE_DEV_COUNTS:
            buf = torch.full((VALUE_BOUND,), float("nan"), dtype=torch.float32, device="cuda")
            n_dev = torch.tensor([count], dtype=torch.int32, device="cuda")
            value.forward_boards_counted(o, p, perm, n_dev, buf)
            out["vd_%d" % count] = bits(buf)
        for n in VALUE_HOST_ROWS:
            out["vh_%d" % n] = bits(value._forward_split((o[:n], p[:n]), o.device))
    value.check_saturation()


def policy_scenes(out, nets):
    import torch
    engine, ops, policy, value, rw = nets
    gold = np.load(os.path.join(GOLDEN, "nets_shipped.npz"))
    for parts in POLICY_PARTS:
        policy.split3_parts = parts
        for n in POLICY_HOST_ROWS:
            o, p = ops.bits_to_tensor(gold["own"][:n]), ops.bits_to_tensor(gold["opp"][:n])
            out["ph_%d_%d" % (parts, n)] = bits(policy.forward_boards_split3(o, p))
        o, p = ops.bits_to_tensor(gold["own"][:POLICY_BOUND]), ops.bits_to_tensor(gold["opp"][:POLICY_BOUND])
        perm = policy_perm().cuda()
        for count in POLICY_DEV_COUNTS:
            n_dev = torch.tensor([count], dtype=torch.int32, device="cuda")
            probs = policy.forward_boards_split3(o, p, index=perm, n=POLICY_BOUND, n_dev=n_dev)
            out["pd_%d_%d" % (parts, count)] = bits(probs[:count])       # (the rows past the count are not written)
    policy.split3_parts = type(policy).split3_parts
    policy.check_saturation()


def tree_state(m, active, tag, out):
    import torch
    t = m.tree
    G, cap = m.n_games, t.capacity
    live = (torch.arange(cap, device="cuda").reshape(1, cap) < t.n_nodes.reshape(G, 1)).reshape(-1, 1)
    out[tag + "nodes"] = torch.where(live, t.nodes, torch.zeros_like(t.nodes)).cpu().numpy().copy()
    out[tag + "n_nodes"], out[tag + "root"] = t.n_nodes.cpu().numpy().copy(), t.root.cpu().numpy().copy()
    out[tag + "v"] = bits(torch.where(live.reshape(-1), t.v, torch.zeros_like(t.v)))
    out[tag + "leaf_value"] = bits(m.leaf_value)
    move, visits = m.best_move(active)
    out[tag + "move"], out[tag + "visits"] = move.cpu().numpy().copy(), visits.cpu().numpy().copy()
    out[tag + "z_log"], out[tag + "z_log_n"] = m.z_log.cpu().numpy().copy(), m.z_log_n.cpu().numpy().copy()
    out[tag + "overflow"] = t.overflow.cpu().numpy().copy()
    out[tag + "ctl3"] = m._ps["ctl"][3:4].cpu().numpy().copy()
    out[tag + "error_flags"] = m.error_flags().cpu().numpy().copy()
    return move


def search_scene(out, nets, G):
    import torch
    engine, ops, policy, value, rw = nets
    own, opp = search_positions(G)
    m = search_engine(G, nets)
    assert m.persistent
    o, p = ops.bits_to_tensor(own), ops.bits_to_tensor(opp)
    active = torch.ones(G, dtype=torch.uint8, device="cuda")
    active[SEARCH_IDLE] = 0
    m.search(o, p, active, SEARCH_SIMS[0])
    mv = tree_state(m, active, "s%d_a_" % G, out).clone()
    mv = torch.where(mv == -2, torch.full_like(mv, -1), mv)
    m.update_with_move(mv, active.clone())
    ops.apply_moves(o, p, mv)
    m.z_log_n.zero_()
    m.search(p, o, active, SEARCH_SIMS[1])
    tree_state(m, active, "s%d_b_" % G, out)
    out["s%d_capacity" % G] = np.array([m.tree.capacity], np.int64)
    # (diagnostic, depends on the schedule: the pairs of boards the net workgroups walked together)
    out["sched_pairs_%d" % G] = m._ps["totals"][3:4].cpu().numpy().copy()
    m.close()


def main():
    dst = sys.argv[1]
    t0 = time.perf_counter()
    out = {"env": np.array(json.dumps({k: v for k, v in sorted(os.environ.items()) if k.startswith("IAGO_")}))}
    rc = 0
    try:
        nets = shipped_nets()
        value_scenes(out, nets)
        policy_scenes(out, nets)
        for G in SEARCH_GAMES:
            search_scene(out, nets, G)
    except BaseException:   # (reported to the test, which fails with it)
        out["error"] = np.array(traceback.format_exc())
        sys.stderr.write(str(out["error"]))
        rc = 1
    out["wall_s"] = np.array([time.perf_counter() - t0])
    np.savez(dst, **out)
    sys.exit(rc)


if __name__ == "__main__":
    main()
