"""Weights that change between launches, engine by engine, and the training loops as they run.  An engine keeps
state across launches that belongs to the weights that computed it: the values stored in the nodes, the persistent
search's position table (shared by every launch of the engine), the look-ahead's cached priors, a captured graph.
After a change of one value-net tensor, then of one policy-net tensor, a launch must give bit for bit what an
engine built fresh on modules loaded from the changed weights gives from the same state (seed, game_id_base,
sim_counter, trees reset) -- the trees, or the records and visit counts of whole games."""
import os

import numpy as np
import pytest
import torch

from tests import table_util
from tests.conftest import GOLDEN, load_json
from tests.gpu_util import delta, fresh, random_positions

pytestmark = pytest.mark.gpu

G, N_SIMS, TURNS, S0 = 8, 24, 10, 1000
TREE = ("n_visits", "q", "p", "first_child", "parent", "action", "n_children", "n_nodes", "root", "v")
GAME = ("own", "opp", "valid", "move", "pi", "z", "final_p1", "final_p2")


def _nets():
    from iago_amd import network
    policy = network.SLPolicy().load_npz(os.path.join(GOLDEN, "sl_model.npz")).cuda().eval()
    value = network.Value().load_npz(os.path.join(GOLDEN, "value_model.npz")).cuda().eval()
    return policy, value


def _rw():
    from iago_amd import ops
    g = load_json("simulate.json")
    return ops.RolloutWeights(g["shipped_w"], g["shipped_b"])


def _change(module, name, seed):
    p = dict(module.named_parameters())[name]
    with torch.no_grad():
        p.add_(delta(p, seed))


def _roots(n):
    from iago_amd import ops
    own, opp = random_positions(n, seed=17)
    own[: n // 2], opp[: n // 2] = 0x0000000810000000, 0x0000001008000000
    return ops.bits_to_tensor(own), ops.bits_to_tensor(opp)


KINDS = {
    "persistent": dict(persistent=True, split=0),
    "split": dict(persistent=True, split=8),
    "wave": dict(persistent=True, wave=8),
    "play": dict(persistent=True, split=0),
    "stream": dict(persistent=True, split=0),
    "match": dict(persistent=True, split=0),
}


def _engine(policy, value, kind, games=G):
    from iago_amd import engine
    m = engine.BatchedMCTS(games, policy, value, _rw(), n_thr=15, capacity=8192, seed=21, game_id_base=300,
                           **KINDS[kind])
    assert m.persistent and m._vtable is not None
    if kind == "split":
        assert m._split is not None and m.split_cus == 8
    if kind == "wave":
        assert m.wave_entry
    return m


def _launch(m, kind):
    """One launch of the kind from the same state (trees reset, sim_counter S0): host copies of what it built."""
    from iago_amd import engine
    m.sim_counter = S0
    m.tree.reset()
    if kind in ("persistent", "split", "wave"):
        o, p = _roots(m.n_games)
        active = torch.ones(m.n_games, dtype=torch.uint8, device="cuda")
        m.search(o, p, active, N_SIMS)
        t = m.tree
        nodes = t.n_nodes.cpu().numpy()
        live = (np.arange(t.capacity).reshape(1, -1) < nodes.reshape(-1, 1)).reshape(-1)   # (the pools' used nodes)
        out = {k: getattr(t, k).cpu().numpy()[live] for k in TREE if k not in ("n_nodes", "root")}
        out["n_nodes"], out["root"] = nodes, t.root.cpu().numpy()
        out["first_child"] = np.where(out["first_child"] < 0, -1, out["first_child"])
        out["v"] = out["v"].view(np.uint32)          # (NaN = never evaluated: compared as bits)
        return out
    e = engine.SelfPlayEngine(m, max_turns=TURNS)
    if kind == "play":
        r = e.play(N_SIMS)
    elif kind == "stream":
        r = e.play_stream(N_SIMS, G + G // 2)
        assert r.launches == 1
    else:
        col = torch.full((G,), 2, dtype=torch.int64, device="cuda")
        col[1::2] = 1
        r = e.play_match(N_SIMS, mcts_colour=col)
        assert r.launches == 1
    out = {k: getattr(r, k).cpu().numpy().copy() for k in GAME}
    out["n_turns"], out["sim"] = r.n_turns, m.sim_counter
    return out


def _equal(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def audit_table(m, value):
    """Every entry of the position table holds, bit for bit, the current value net's value of its position (the
    one-board walk: what a launch would take from it), every entry in use walked -- and is a published entry of one of
    the launch's writers in the slot a lookup reads (tests/table_util.py).  Returns the entries in use."""
    n_used, n_walked = table_util.audit(m, value)
    assert n_walked == n_used
    return n_used


@pytest.mark.parametrize("kind", list(KINDS))
def test_launches_follow_weight_changes(kind):
    policy, value = _nets()
    m = _engine(policy, value, kind)
    first = _launch(m, kind)
    assert audit_table(m, value) > 0                       # the table holds entries of these weights
    for net, name, seed in ((value, "block4.conv.weight", 1), (policy, "block3.conv.bias", 2)):
        _change(net, name, seed)
        got = _launch(m, kind)
        if net is value:
            audit_table(m, value)                          # nothing of the old weights is left in the table
        f = _engine(fresh(policy), fresh(value), kind)
        want = _launch(f, kind)
        f.close()
        _equal(got, want)
        assert any(not np.array_equal(got[k], first[k]) for k in got if k not in ("n_turns", "sim")), name
        first = got
    m.close()


def test_position_table_after_a_value_change_holds_no_old_value():
    """The same roots searched on an empty table, then on the warm table (its entries answer), then right after a
    value change, then once more on the new weights' warm table; the trees reset before each search.  The search
    after the change must count table hits like a search on an empty table -- a fresh engine's first search on the
    new weights (the same trees) -- not like one on a warm table, and every entry in use afterwards holds a value of
    the new weights."""
    policy, value = _nets()
    games = 64
    m = _engine(policy, value, "persistent", games)
    hits, trees = [], None
    for change in (False, False, True, False):
        if change:
            _change(value, "fc11.weight", 3)
        t0 = m._ps["totals"][8].item()
        out = _launch(m, "persistent")
        trees = out if change else trees
        hits.append(int(m._ps["totals"][8].item() - t0))        # totals[8]: position-table hits
        assert audit_table(m, value) > 0
    f = _engine(fresh(policy), fresh(value), "persistent", games)
    _equal(trees, _launch(f, "persistent"))
    fresh_hits = int(f._ps["totals"][8].item())
    f.close()
    first, warm, after, warm_after = hits
    print("table hits: empty table %d, warm table %d, after the value change %d, its warm table %d, fresh engine %d"
          % (first, warm, after, warm_after, fresh_hits))
    # (hits among a search's own entries depend on the order in which the games reach shared positions: two searches
    # on empty tables agree only roughly; a warm table answers many more requests)
    assert warm > first and warm_after > fresh_hits
    assert abs(after - fresh_hits) < abs(after - warm_after)
    m.close()


def test_lookahead_priors_follow_a_policy_change():
    """The per-playout engine with the policy look-ahead caches the priors of leaves a few visits before they
    expand; a policy change between two searches of the same trees (no reset) must not let those leaves expand with
    the old priors: the trees equal those of the reference order of evaluation (the net at the expansion)."""
    from iago_amd import engine
    policy, value = _nets()
    rw = _rw()
    n = 32

    def make(lookahead):
        return engine.BatchedMCTS(n, policy, value, rw, n_thr=15, capacity=8192, seed=13, sync_free=True,
                                  persistent=False, lookahead=lookahead)

    ref, la = make(0), make(4)
    assert ref.lookahead == 0 and la.lookahead == 4 and not la.persistent
    o, p = _roots(n)
    steps = [(50, None), (37, "block2.conv.weight"), (41, "bias10.b"), (30, "block6.conv.bias")]
    idle = torch.ones(n, dtype=torch.uint8, device="cuda")
    idle[3::8] = 0          # games that sit out the search right after the first change (their priors stay stale)
    for t, (n_sims, change) in enumerate(steps):
        if change is not None:
            _change(policy, change, t)
        active = idle if t == 1 else torch.ones(n, dtype=torch.uint8, device="cuda")
        ref.search(o, p, active, n_sims)
        la.search(o, p, active, n_sims)
        for g in range(n):
            assert ref.tree.dump(g, max_depth=64) == la.tree.dump(g, max_depth=64), (t, g)
        if t + 1 < len(steps):
            # leaves whose priors the look-ahead cached are waiting when the weights change before the next search
            assert cached_leaves(la) > 0, t
        if t == 1:
            # the games that sat out still wait with priors of the old weights, refreshed when they search again
            assert bool(la._la_stale[idle == 0].all()) and not bool(la._la_stale[idle != 0].any())
            assert cached_leaves(la, idle == 0) > 0


def cached_leaves(m, games=None):
    """Unexpanded leaves of m's trees (of the games of the mask `games`, default all) whose priors sit in the look-ahead's cache (tag and cache slot agree, as
    iago_mcts_expand_cached reads them)."""
    t, S = m.tree, m._la[0].slots
    fc = t.first_child.reshape(t.n_games, t.capacity)
    seq = (-2 - fc).clamp(min=0)
    live = torch.arange(t.capacity, device=fc.device).reshape(1, -1) < t.n_nodes.reshape(-1, 1)
    cached = m._la_cache_seq.gather(1, (seq % S).to(torch.int64)) == seq
    pick = live & (fc <= -2) & cached
    if games is not None:
        pick &= games.reshape(-1, 1)
    return int(pick.sum().item())


def test_pv_mcts_round_on_the_same_engine():
    """SelfPlayEngine.play -> ReinforceTrainer.step_from_tuples -> play on the SAME engine equals a fresh engine on
    the learner's updated weights."""
    from iago_amd import engine
    from iago_amd.train_rl import ReinforceTrainer
    policy, value = _nets()
    tr = ReinforceTrainer(policy, pool_dir=None, N=G, seed=4)
    tr.model1.eval()
    m = _engine(tr.model1, value, "play")
    e = engine.SelfPlayEngine(m, max_turns=TURNS)
    m.sim_counter = S0
    first = e.play(N_SIMS)
    tr.step_from_tuples(first.tuples())
    tr.model1.eval()
    got = _launch(m, "play")
    f = _engine(fresh(tr.model1), fresh(value), "play")
    _equal(got, _launch(f, "play"))
    assert not np.array_equal(got["pi"], first.pi.cpu().numpy())
    f.close()
    m.close()


def test_reinforce_sets_against_itself():
    """ReinforceTrainer with no pool: the learner plays both colours; after two step() calls play_set equals that of
    a freshly built module on the learner's weights."""
    from iago_amd.train_rl import ReinforceTrainer
    policy, _ = _nets()
    tr = ReinforceTrainer(policy, pool_dir=None, N=8, seed=6)
    tr.step()
    tr.step()
    assert tr.opt.t == 2
    idx, rs = tr.set_index, tr.rs.get_state()
    got, wins = tr.play_set(tr.pick_opponent())
    tr2 = ReinforceTrainer(fresh(tr.model1), pool_dir=None, N=8, seed=6)
    tr2.set_index = idx
    tr2.rs.set_state(rs)
    want, wins2 = tr2.play_set(tr2.pick_opponent())
    assert wins == wins2 and set(got) == set(want)
    for k in got:
        assert torch.equal(got[k], want[k]), k


def test_supervised_native_epoch():
    """After one native supervised epoch of the Value net, evaluate and value_grads equal a fresh module's."""
    from iago_amd import ops
    from iago_amd.train_supervised import SupervisedTrainer
    _, value = _nets()
    own, opp = random_positions(600, seed=23)
    o, p = ops.bits_to_tensor(own), ops.bits_to_tensor(opp)
    z = (torch.arange(600, device="cuda") % 3 - 1).to(torch.float32)
    tr = SupervisedTrainer(value, "value", seed=3, native=True)
    warm = tr.evaluate(o, p, z)
    value.value_grads(o[:64], p[:64], z[:64])
    assert "_split_cache" in value.__dict__ and "_bwd_cache" in value.__dict__ and "_head_cache" in value.__dict__
    tr.epoch(o, p, z)
    assert tr.opt.t == 1
    f = fresh(value)
    got, want = tr.evaluate(o, p, z), SupervisedTrainer(f, "value", native=True).evaluate(o, p, z)
    assert got == want and got != warm
    with torch.no_grad():
        assert torch.equal(value(ops.encode_planes(o, p)), f(ops.encode_planes(o, p)))
    la, lb = value.value_grads(o[:64], p[:64], z[:64]), f.value_grads(o[:64], p[:64], z[:64])
    assert torch.equal(la, lb)
    for (n, a), b in zip(value.named_parameters(), f.parameters()):
        assert torch.equal(a.grad, b.grad), n
