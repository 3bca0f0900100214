"""The kernel forms that only an environment knob selects (LABNOTES.md section 5, "Tuning knobs": "all give the same
results").

Knobs that the library latches on first use run in a child process each (tests/knob_worker.py: fixed scenes from fixed
seeds, one .npz): the default child is pinned to the references first -- the float64 outputs of oracle/nets_np.py for
the two shipped nets (tests/golden/nets_shipped.npz and the oracle itself, tolerance of tests/test_nets_shipped.py) and
the tree of oracle/mcts_py.py for the 20-game search (as tests/test_mcts_production_gpu.py builds it) -- and every
setting's child must then equal the default child bit for bit, NaN tails included.  The children run strictly one
after another (the parent and one child hold the device at a time); a child that faults, aborts or runs into its time
limit fails every later case of this module at once, without anything more being started on the device.

Knobs read per call or by Python run in-process under monkeypatch.setenv.
"""
import json
import os
import subprocess
import sys
import time
import types

import numpy as np
import pytest
import torch

from tests import knob_worker as kw
from tests.conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

WORKER = os.path.join(ROOT, "tests", "knob_worker.py")
TOL = 1e-5                        # tests/test_nets_shipped.py: BASELINE.json north_star, probabilities and the Value scalar
# wall time of the default child on one MI355X, measured (LABNOTES.md, "Knob forms": 2.7 s, of which 2.2 s in the
# scenes -- process start, torch and HIP initialisation included).  A child may take three times the default child's:
# the recorded figure, or what the default child of this very run took where that was longer (a busier machine)
DEFAULT_CHILD_WALL_S = 2.7
_default_wall = [DEFAULT_CHILD_WALL_S]

SETTINGS = [
    {"IAGO_VALUE_PERSIST": "0"},
    {"IAGO_VALUE_PERSIST": "0", "IAGO_VALUE_TINY": "3"},
    {"IAGO_VALUE_TINY": "0"},
    {"IAGO_VALUE_TINY": "1000"},
    {"IAGO_VALUE_PERSIST": "0", "IAGO_VALUE_TINY": "1000"},
    {"IAGO_POLICY_GRID": "1"},
    {"IAGO_POLICY_GRID": "5"},
    {"IAGO_PERSISTENT_PAIR": "0"},
    {"IAGO_PERSISTENT_PAIR": "64"},
    {"IAGO_PERSISTENT_POLICY_XCDS": "0"},
    {"IAGO_PERSISTENT_POLICY_XCDS": "7"},
]

_FAULT = []      # the first child that faulted: every later case fails without touching the device


def _run_child(tmp, setting):
    """One worker process under `setting` (every other IAGO_* variable removed, but for the library to load); returns
    its arrays."""
    if _FAULT:
        pytest.fail("not started: an earlier child faulted (%s)" % _FAULT[0])
    env = {k: v for k, v in os.environ.items() if not k.startswith("IAGO_") or k == "IAGO_HIP_LIB"}
    env.update(setting)
    name = "_".join("%s=%s" % kv for kv in sorted(setting.items())) or "default"
    dst = os.path.join(str(tmp), name + ".npz")
    limit = 3 * _default_wall[0]
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, WORKER, dst], env=env, cwd=ROOT, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        _FAULT.append("%s: no end within %.1f s" % (name, limit))
        pytest.fail(_FAULT[0])
    wall = time.perf_counter() - t0
    if not setting:
        _default_wall[0] = max(_default_wall[0], wall)
    if r.returncode in (-6, -11, 134, 139) or "illegal memory access" in r.stderr:
        _FAULT.append("%s: exit status %d\n%s" % (name, r.returncode, r.stderr[-2000:]))
        pytest.fail(_FAULT[0])
    assert r.returncode == 0 and os.path.exists(dst), (name, r.returncode, r.stderr[-4000:])
    d = dict(np.load(dst))
    assert "error" not in d, str(d.get("error"))
    seen = json.loads(str(d["env"]))
    seen.pop("IAGO_HIP_LIB", None)
    assert seen == setting                               # (the child saw this setting and no other knob)
    print("knob child %s: %.1f s wall, %.1f s of it in the scenes; pairs walked %s"
          % (name, wall, float(d["wall_s"][0]), [int(d["sched_pairs_%d" % G][0]) for G in kw.SEARCH_GAMES]))
    return d


@pytest.fixture(scope="module")
def default_child(tmp_path_factory):
    return _run_child(tmp_path_factory.mktemp("knobs"), {})


@pytest.fixture(autouse=True)
def _nothing_after_a_fault():
    if _FAULT:
        pytest.fail("not started: an earlier child faulted (%s)" % _FAULT[0])


def _f32(a):
    return a.view(np.float32)


def _no_errors(d):
    for G in kw.SEARCH_GAMES:
        for stage in "ab":
            tag = "s%d_%s_" % (G, stage)
            assert not d[tag + "overflow"].any(), tag
            assert int(d[tag + "ctl3"][0]) == 0, tag                       # no launch gave up at its clock limit
            assert d[tag + "error_flags"].tolist() == [0, 0, 0, 0, 0], tag


# ------------------------------------------------------------------ the default child against the references

def test_default_value_forward_vs_float64(default_child):
    """Host-counted and device-counted Value forwards of the default child against the float64 oracle: the 256 golden
    positions through the committed outputs, a sample of the other rows through oracle/nets_np.py itself; the rows of a
    device count are written, the others keep their NaN; a board's value does not depend on the batch it came in."""
    from oracle import nets_np
    from tests.test_nets_shipped import planes_np
    d = default_child
    gold = np.load(os.path.join(GOLDEN, "nets_shipped.npz"))
    own, opp = kw.value_positions()
    want = np.full(kw.VALUE_BOUND, np.nan)
    want[:256] = gold["value"]
    sample = np.arange(256, kw.VALUE_BOUND, 23)
    want[sample] = nets_np.value(planes_np(own[sample], opp[sample]), dict(np.load(os.path.join(GOLDEN, "value_model.npz"))))
    known = ~np.isnan(want)
    full = _f32(d["vh_%d" % kw.VALUE_BOUND])
    err = np.max(np.abs(full[known] - want[known]))
    print("default child, Value host-counted %d rows: max |error| to float64 %.3g" % (kw.VALUE_BOUND, err))
    assert err < TOL, err
    for n in kw.VALUE_HOST_ROWS:
        got = _f32(d["vh_%d" % n])
        assert got.shape == (n,)
        k = known[:n]
        assert np.max(np.abs(got[k] - want[:n][k])) < TOL, n
        assert np.array_equal(d["vh_%d" % n], d["vh_%d" % kw.VALUE_BOUND][:n]), n      # (the same bits in every batch)
    perm = kw.value_perm().numpy()
    nan_bits = np.full(1, np.nan, np.float32).view(np.uint32)[0]
    for count in kw.VALUE_DEV_COUNTS:
        got = d["vd_%d" % count]
        rows, rest = perm[:count], perm[count:]
        assert np.all(got[rest] == nan_bits), count                         # untouched, bit for bit
        assert not np.isnan(_f32(got)[rows]).any(), count                  # written
        k = rows[known[rows]]
        assert k.size == 0 or np.max(np.abs(_f32(got)[k] - want[k])) < TOL, count
        assert np.array_equal(got[rows], d["vh_%d" % kw.VALUE_BOUND][rows]), count


def test_default_policy_forward_vs_float64(default_child):
    """forward_boards_split3 of the default child against the committed float64 move distributions."""
    d = default_child
    gold = np.load(os.path.join(GOLDEN, "nets_shipped.npz"))
    perm = kw.policy_perm().numpy()
    for parts in kw.POLICY_PARTS:
        for n in kw.POLICY_HOST_ROWS:
            got = _f32(d["ph_%d_%d" % (parts, n)])
            assert got.shape == (n, 64)
            err = np.max(np.abs(got - gold["sl_probs"][:n]))
            assert err < TOL, (parts, n, err)
            assert np.array_equal(got.argmax(axis=1), gold["sl_probs"][:n].argmax(axis=1))
        for count in kw.POLICY_DEV_COUNTS:
            got = _f32(d["pd_%d_%d" % (parts, count)])
            assert got.shape == (count, 64)
            if count:
                assert np.max(np.abs(got - gold["sl_probs"][perm[:count]])) < TOL, (parts, count)


def _dump(d, tag, G, g):
    """Game g's tree of a saved search in the format of oracle.mcts_py.dump_tree (TreePool.dump on the saved arrays)."""
    from iago_amd import engine
    pool = types.SimpleNamespace(capacity=int(d["s%d_capacity" % G][0]), n_nodes=torch.from_numpy(d[tag + "n_nodes"]),
                                 nodes=torch.from_numpy(d[tag + "nodes"]), root=torch.from_numpy(d[tag + "root"]))
    return engine.TreePool.dump(pool, g, max_depth=64)


def test_default_search_vs_oracle(default_child):
    """The 20-game persistent search of the default child against oracle/mcts_py.MCTS, fed the rollout results the
    search recorded and the nets' outputs from the production kernels on single boards (tests/test_mcts_production_gpu.py):
    trees bit for bit, moves and visit counts, after the first search and after update_with_move + the second."""
    from oracle import mcts_py
    from oracle import oracle as orc
    from tests.gpu_util import state_of
    from tests.test_mcts_production_gpu import NetProbe
    from tests.test_oracle_golden import _cmp_tree
    d = default_child
    _no_errors(d)
    G = 20
    n1, n2 = kw.SEARCH_SIMS
    nets = kw.shipped_nets()
    probe = NetProbe(nets[1], nets[2], nets[3])
    own, opp = kw.search_positions(G)
    a, b = "s%d_a_" % G, "s%d_b_" % G
    zn = d[a + "z_log_n"]
    assert zn[kw.SEARCH_IDLE] == 0 and np.all(np.delete(zn, kw.SEARCH_IDLE) == n1)
    assert np.all(np.delete(d[b + "z_log_n"], kw.SEARCH_IDLE) == n2)
    assert d[a + "n_nodes"][kw.SEARCH_IDLE] == 1
    move, visits = d[a + "move"], d[a + "visits"]
    for g in (0, 1, 2, 9, 10, 11, 12):
        it = iter(d[a + "z_log"][:n1, g])
        om = mcts_py.MCTS(probe.policy_fn, probe.value_fn, lambda s, c, it=it: int(next(it)), lmbda=0.5, c_puct=1.0, n_thr=15)
        want_move = om.get_move(state_of(own[g], opp[g]), 1, n1)
        assert next(it, None) is None
        _cmp_tree(_dump(d, a, G, g), mcts_py.dump_tree(om.root, max_depth=64), "g%d" % g)
        if want_move is None:
            assert move[g] == -2
        else:
            assert move[g] == want_move, g
            for act, ch in om.root.children.items():
                if act >= 0:
                    assert visits[g, act] == ch.n_visits
        mv = -1 if move[g] == -2 else int(move[g])
        om.update_with_move(mv)
        s = state_of(own[g], opp[g])
        orc.place_stone(s, mv, 1)
        it = iter(d[b + "z_log"][:n2, g])
        om.rollout_fn = lambda st, c, it=it: int(next(it))
        om.get_move(s, 2, n2)
        _cmp_tree(_dump(d, b, G, g), mcts_py.dump_tree(om.root, max_depth=64), "g%d'" % g)
    # the larger search took part: every game but the idle one ran its playouts and grew a tree
    zn = d["s96_b_z_log_n"]
    assert np.all(np.delete(zn, kw.SEARCH_IDLE) == n2) and np.all(np.delete(d["s96_b_n_nodes"], kw.SEARCH_IDLE) > 1)


# ------------------------------------------------------------------ one child per setting

@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: " ".join("%s=%s" % kv for kv in s.items()))
def test_setting_gives_the_default_results(default_child, setting, tmp_path):
    """Every scene of a child under `setting` equals the default child's bit for bit -- what the comments at the knobs
    and the LABNOTES table claim: the windowed device-counted Value forward (IAGO_VALUE_PERSIST=0) at the counts around
    its windows' edges, the one- / two-board threshold IAGO_VALUE_TINY at 0, 3 and beyond the four-board threshold
    (clamped to it), a policy grid of 1 and of 5 workgroups walking several rows each, and the persistent search with
    the pair walk off / rare and the policy ring's home XCDs none / all but one -- and no overflow word is set, no
    launch gave up."""
    d = _run_child(tmp_path, setting)
    _no_errors(d)
    compared = [k for k in sorted(d) if k not in ("env", "wall_s") and not k.startswith("sched_")]
    assert compared == [k for k in sorted(default_child) if k not in ("env", "wall_s") and not k.startswith("sched_")]
    assert len(compared) > 60
    for k in compared:
        assert d[k].dtype == default_child[k].dtype and np.array_equal(d[k], default_child[k]), k
    if setting.get("IAGO_PERSISTENT_PAIR") == "0":
        assert all(int(d["sched_pairs_%d" % G][0]) == 0 for G in kw.SEARCH_GAMES)      # (the pair walk was off)


# ------------------------------------------------------------------ knobs read per call or by Python

def _trunk_case(ops, n, cin, n_layers):
    g = torch.Generator().manual_seed(1000 * n + 10 * cin + n_layers)
    x0 = (torch.rand(n, cin, 8, 8, generator=g) * 2).cuda()
    layers, f64, c = [], [], cin
    for _ in range(n_layers):
        w = (torch.randn(128, c, 3, 3, generator=g) / np.sqrt(9 * c)).cuda()
        b = (torch.randn(128, generator=g) * 0.1).cuda()
        layers.append(ops.split_weights(w) + (b,))
        f64.append((w.double(), b.double()))
        c = 128
    want = x0.double()
    for w, b in f64:
        want = torch.relu(torch.nn.functional.conv2d(want, w, b, padding=1))
    return x0, layers, want


@pytest.mark.parametrize("n_layers", [1, 3, 8])
@pytest.mark.parametrize("cin", [64, 128])
def test_staged_trunk(cin, n_layers, monkeypatch):
    """IAGO_TRUNK_STAGED=1: iago_conv3x3_split_trunk as the round-1 LDS-staged kernel (conv3x3_split_trunk_kernel), at
    1, 4, 5 and 37 boards (one board, a full workgroup of 4, one more, ten workgroups with a ragged last one), against
    a float64 convolution of the same operands at the tolerance of test_conv_gpu.py's trunk test, and bit for bit
    against the per-layer launches (the staged trunk runs the per-layer kernel's conv_layer on every layer).  Unset
    and "0" select the resident trunk (the table's default), which sums a product's input channels in another order
    (test_trunk_kernel_equals_layer_by_layer): staged and resident are not bit-identical.  Measured over these cases:
    |staged - resident| at most 2.9e-6 at activations up to 5.4 (5e-7 of the largest activation), each within 2.5e-6 of
    the float64 result."""
    from iago_amd import ops
    for n in (1, 4, 5, 37):
        x0, layers, want = _trunk_case(ops, n, cin, n_layers)
        a0 = ops.split_nchw(x0)
        monkeypatch.delenv("IAGO_TRUNK_STAGED", raising=False)
        resident = ops.merge_nchw(ops.conv3x3_split_trunk(a0, layers))
        monkeypatch.setenv("IAGO_TRUNK_STAGED", "0")
        assert torch.equal(ops.merge_nchw(ops.conv3x3_split_trunk(a0, layers)), resident)    # 0 = unset
        monkeypatch.setenv("IAGO_TRUNK_STAGED", "1")
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        staged = ops.merge_nchw(ops.conv3x3_split_trunk(a0, layers, overflow=flag))
        monkeypatch.delenv("IAGO_TRUNK_STAGED")
        assert int(flag.item()) == 0
        ref = a0
        for w_hi, w_lo, b in layers:
            ref = ops.conv3x3_split(ref, w_hi, w_lo, b)
        per_layer = ops.merge_nchw(ref)
        scale = float(want.abs().max())
        es, er = float((staged.double() - want).abs().max()), float((resident.double() - want).abs().max())
        diff = float((staged - resident).abs().max())
        print("staged trunk n=%d cin=%d layers=%d: |staged - f64| %.3g, |resident - f64| %.3g, |staged - resident| %.3g, "
              "scale %.3g" % (n, cin, n_layers, es, er, diff, scale))
        assert es < 2e-5 * scale and er < 2e-5 * scale, (n, es, er, scale)
        assert torch.equal(staged, per_layer), n
        assert n < 37 or n_layers < 3 or diff > 0.0      # (the knob did select another kernel)


def _lockstep_engines(monkeypatch, knob, value, **kw_):
    """The default per-playout engine and the one under `knob`, on the same random-init nets (tests/test_mcts_gpu.py's
    smallest look-ahead case: 16 games, pools of 512 nodes)."""
    from iago_amd import engine, network, ops
    from tests.conftest import load_json
    g = load_json("simulate.json")
    torch.manual_seed(4)
    policy, value_net = network.SLPolicy().cuda().eval(), network.Value().cuda().eval()
    w = ops.RolloutWeights(g["shipped_w"], g["shipped_b"])

    def make(env):
        if env:
            monkeypatch.setenv(knob, value)
        m = engine.BatchedMCTS(16, policy, value_net, w, n_thr=15, capacity=512, seed=13, lookahead=4, **kw_)
        if env:
            monkeypatch.delenv(knob)
        return m

    return ops, make(False), make(True)


def _same_trees(ops, ms, n_sims=45):
    from tests.gpu_util import random_positions
    G, cap = 16, 512
    own, opp = random_positions(G, seed=8)
    own[:4], opp[:4] = 0x0000000810000000, 0x0000001008000000
    boards = [(ops.bits_to_tensor(own), ops.bits_to_tensor(opp)) for _ in ms]
    used = torch.arange(cap, device="cuda").reshape(1, cap)
    for t in range(2):
        active = (ops.legal_moves(*boards[0]) != 0).to(torch.uint8)
        for m, (o, p) in zip(ms, boards):
            m.search(o, p, active, n_sims)
            assert m.error_flags().tolist() == [0, 0, 0, 0, 0], t
        ref = ms[0]
        live = (used < ref.tree.n_nodes.reshape(G, 1)).reshape(-1)
        assert int((ref.tree.n_nodes > 1).sum().item()) >= G // 2   # (the expansions did run)
        for m in ms[1:]:
            assert torch.equal(m.tree.n_nodes, ref.tree.n_nodes), t
            assert torch.equal(m.tree.root, ref.tree.root), t
            assert torch.equal(m.tree.nodes[live], ref.tree.nodes[live]), t
            assert torch.equal(m.leaf_value.view(torch.int32), ref.leaf_value.view(torch.int32)), t
        mv = ref.best_move(active)[0]
        mv = torch.where(active.bool(), mv, torch.full_like(mv, -1))
        for i, (m, (o, p)) in enumerate(zip(ms, boards)):
            ops.apply_moves(o, p, mv)
            m.update_with_move(mv)
            boards[i] = (p, o)


def test_split_leaf_evaluation_builds_the_same_trees(monkeypatch):
    """IAGO_FUSED_LEAF_EVAL=0: the Value rows and the rollouts of a playout as two launches instead of
    value_rollout_kernel's one -- bit-identical pools, roots and leaf values over two searches with subtree reuse,
    against the default (which tests/test_mcts_production_gpu.py pins to the oracle)."""
    ops, ref, m = _lockstep_engines(monkeypatch, "IAGO_FUSED_LEAF_EVAL", "0")
    assert ref.fused_leaf_eval is True and m.fused_leaf_eval is False
    assert ref.lookahead == m.lookahead == 4 and ref.value_cache and m.value_cache
    _same_trees(ops, [ref, m])


def test_graph_blocks_build_the_same_trees(monkeypatch):
    """IAGO_GRAPH_BLOCKS=1: the long graph of a replayed search holds one look-ahead block (8 playouts) instead of four
    -- 45 playouts are 1 x 32 + 1 x 8 + 5 by default and 5 x 8 + 5 under the knob: the same trees."""
    ops, ref, m = _lockstep_engines(monkeypatch, "IAGO_GRAPH_BLOCKS", "1", use_graph=True)
    assert ref.graph_blocks == 4 and m.graph_blocks == 1 and ref.use_graph and m.use_graph
    _same_trees(ops, [ref, m])
    assert ref._graph is not None and m._graph is not None       # (both replayed)


def test_side_stream_priority_builds_the_same_trees(monkeypatch):
    """IAGO_SIDE_PRIORITY=-1: the policy batches' side stream at high priority: the same trees."""
    ops, ref, m = _lockstep_engines(monkeypatch, "IAGO_SIDE_PRIORITY", "-1")
    assert ref._la_side.priority == 0 and m._la_side.priority == -1
    _same_trees(ops, [ref, m])
