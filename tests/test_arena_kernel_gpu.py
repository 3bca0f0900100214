"""The arena launch (iago_mcts_search_arena, include/iago_hip_serving.h; ops.search_arena): two persistent searches, each
with its own nets, trees, rings and constants, in ONE grid.  What must hold: each agent's pool, moves, visit rows and
evaluation counts are those of iago_mcts_search_persistent run alone on a twin engine (same nets, seeds, ids,
sim_counter), bit for bit -- at 24 + 8 roots (3 + 1 game workgroups of 8 games: the smallest shape at which a wrong
workgroup index for agent B shows) and swapped; B's trees really come from B's nets; a side without work hands its
workgroups over (2 and 5 net workgroups: one server per agent); the constants are per agent; the trees are
oracle/mcts_py.MCTS's; and what the entry point documents as refused is refused with nothing launched.

The evaluation counts: totals[1] (policy) is a function of the trees.  totals[0] (value requests) is one only without
the position table -- with it a fresh leaf is asked for OR found in the table (totals[8]), whichever game got there
first -- so the comparison runs both ways: table off, totals[0..1] themselves; table on (the default), totals[0] +
totals[8] and totals[1]."""
import numpy as np
import pytest
import torch

from oracle import mcts_py
from tests.conftest import load_json
from tests.gpu_util import random_positions, state_of
from tests.test_mcts_production_gpu import NetProbe
from tests.test_oracle_golden import _cmp_tree

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

N_THR = 2          # (at the default 15 no root expands in 16 playouts)
POOL = ("nodes", "n_nodes", "root", "overflow")


@pytest.fixture(scope="module")
def nets():
    from iago_amd import engine, network, ops
    assert torch.cuda.is_available()
    pairs = {}
    for name, seed in (("a", 3), ("b", 4)):
        torch.manual_seed(seed)
        pairs[name] = (network.SLPolicy().cuda().eval(), network.Value().cuda().eval())   # random init, split paths
    g = load_json("simulate.json")
    return engine, ops, pairs, ops.RolloutWeights(g["shipped_w"], g["shipped_b"])


@pytest.fixture(scope="module")
def roots(golden_rules):
    """32 roots from oracle random play at mixed depths, a must-pass, a dead and a full board and near-end positions
    among them; two of them inactive."""
    own, opp = random_positions(32, seed=41)
    eb = golden_rules["edge_boards"]
    for k, e in ((1, 6), (2, 5), (3, 8), (25, 6), (27, 5)):   # 'pass1', 'dead', 'full'
        own[k], opp[k] = eb[e][0], eb[e][1]
    late, at = random_positions(64, seed=42), [4, 6, 28, 30]
    empties = np.array([64 - bin(int(o) | int(p)).count("1") for o, p in zip(*late)])
    for k, j in zip(at, np.argsort(empties)[2:6]):            # (a few of the emptiest-but-not-over)
        own[k], opp[k] = late[0][j], late[1][j]
    active = np.ones(32, np.uint8)
    active[[5, 26]] = 0
    return own, opp, active


def _engine(nets, net, who, G, n_sims, **kw):
    """Agent `who`'s engine (its seed and ids) on the nets of pair `net`."""
    engine, ops, pairs, rw = nets
    policy, value = pairs[net]
    kw.setdefault("lmbda", 0.5)
    m = engine.BatchedMCTS(G, policy, value, rw, n_thr=N_THR, capacity=engine.suggest_capacity(n_sims, N_THR, moves=2),
                           seed=21 if who == "a" else 22, game_id_base=300 if who == "a" else 7000, persistent=True,
                           z_log_rows=n_sims, **kw)
    m.sim_counter = 1000 if who == "a" else 5000
    assert m.persistent and m.games_per_workgroup == 8 and m._split is None
    return m


def _dev(ops, roots, lo, hi):
    own, opp, active = roots
    return (ops.bits_to_tensor(own[lo:hi]), ops.bits_to_tensor(opp[lo:hi]),
            torch.tensor(active[lo:hi], dtype=torch.uint8, device="cuda"))


def _snap(m, active):
    torch.cuda.synchronize()
    assert int(m._ps["ctl"][3].item()) == 0            # (it did not give up)
    t = m.tree
    out = {k: getattr(t, k).cpu().numpy().copy() for k in POOL}
    move, visits = m.best_move(active)
    on = active.cpu().numpy() != 0
    out["move"], out["visits"] = move.cpu().numpy()[on].copy(), visits.cpu().numpy()[on].copy()
    tot = m._ps["totals"].cpu().numpy()
    out["policy_evals"], out["value_evals"], out["fresh_leaves"] = int(tot[1]), int(tot[0]), int(tot[0] + tot[8])
    out["z_log"], out["z_log_n"] = m.z_log.cpu().numpy().copy(), m.z_log_n.cpu().numpy().copy()
    out["leaf_value"] = m.leaf_value.cpu().numpy()[on].copy()
    return out


def _alone(nets, net, who, r, n_sims, **kw):
    """The twin: iago_mcts_search_persistent alone."""
    m = _engine(nets, net, who, r[0].numel(), n_sims, **kw)
    m.search(r[0], r[1], r[2], n_sims)
    return _snap(m, r[2])


def _arena(nets, ra, rb, n_a, n_b, net_workgroups=None, kw_a=None, kw_b=None):
    """ONE iago_mcts_search_arena of agent A on roots ra and agent B on roots rb -> both engines and their snapshots."""
    ops = nets[1]
    ma = _engine(nets, "a", "a", ra[0].numel(), n_a, **(kw_a or {}))
    mb = _engine(nets, "b", "b", rb[0].numel(), n_b, **(kw_b or {}))
    games = sum(-(-m.n_games // m.games_per_workgroup) for m in (ma, mb))
    net = min(net_workgroups or max(ma.net_workgroups, mb.net_workgroups), ma.resident_workgroups - games)
    keep = []
    args = []
    for m, r, n in ((ma, ra, n_a), (mb, rb, n_b)):
        m._forget_stale_values()
        m.reserve_net_rows(games + net)
        a, k = m._search_args(r[0], r[1], r[2], n)
        a.net_workgroups = net
        args.append(a)
        keep.append(k)
    ops.search_arena(args[0], args[1])
    torch.cuda.synchronize()
    assert int(ma._ps["ctl"][7].item()) == int(mb._ps["ctl"][7].item()) == net   # (the net workgroups it was given)
    del keep
    return (ma, _snap(ma, ra[2])), (mb, _snap(mb, rb[2]))


def _same(got, want, table, who):
    for k in POOL + ("move", "visits", "z_log", "z_log_n", "leaf_value", "policy_evals"):
        assert np.array_equal(got[k], want[k], equal_nan=(k == "leaf_value")), (who, k)
    k = "fresh_leaves" if table else "value_evals"
    assert got[k] == want[k] and got[k] > 0, (who, k, got[k], want[k])


@pytest.fixture(scope="module")
def split_24_8(nets, roots):
    """A: roots 0..23, B: roots 24..31, 16 playouts each, the position tables on (the default): the arena's snapshots
    and the twins'."""
    ops = nets[1]
    ra, rb = _dev(ops, roots, 0, 24), _dev(ops, roots, 24, 32)
    (ma, a), (mb, b) = _arena(nets, ra, rb, 16, 16)
    return dict(ra=ra, rb=rb, ma=ma, mb=mb, a=a, b=b, twin_a=_alone(nets, "a", "a", ra, 16), twin_b=_alone(nets, "b", "b", rb, 16))


def test_bit_identity_24_and_8(split_24_8):
    s = split_24_8
    assert s["ma"].n_games == 24 and s["mb"].n_games == 8
    _same(s["a"], s["twin_a"], True, "A")
    _same(s["b"], s["twin_b"], True, "B")
    # (searched and idle games both: an inactive game's pool is a lone root)
    assert s["a"]["n_nodes"][5] == 1 and s["b"]["n_nodes"][2] == 1 and s["a"]["n_nodes"].max() > 16


def test_bit_identity_swapped_sizes_without_the_table(nets, roots, monkeypatch):
    """A 8 roots, B 24; the position tables off: totals[0..1] themselves are the twins'."""
    monkeypatch.setenv("IAGO_PERSISTENT_TABLE", "0")
    ops = nets[1]
    ra, rb = _dev(ops, roots, 0, 8), _dev(ops, roots, 8, 32)
    (ma, a), (mb, b) = _arena(nets, ra, rb, 16, 16)
    assert ma._vtable is None and mb._vtable is None
    _same(a, _alone(nets, "a", "a", ra, 16), False, "A")
    _same(b, _alone(nets, "b", "b", rb, 16), False, "B")


def test_b_searches_with_its_own_nets(nets, split_24_8):
    """B's seeds, ids and roots on A's nets: other trees -- the arena's B cannot have been served A's weights."""
    s = split_24_8
    other = _alone(nets, "a", "b", s["rb"], 16)
    cap = s["mb"].tree.capacity
    differ = [g for g in range(8) if not np.array_equal(s["b"]["nodes"][g * cap:(g + 1) * cap], other["nodes"][g * cap:(g + 1) * cap])]
    assert differ, "B's trees equal those of A's nets in every game"


@pytest.mark.parametrize("net_workgroups", [None, 2, 5])
def test_hand_over_from_an_agent_without_work(nets, roots, split_24_8, net_workgroups):
    """A's mask empty: its workgroups find A's search over at once and move to B's rings.  With 2 (and 5: an odd
    count) net workgroups each agent has one (two / three) home servers, and A's must move over for B to be served by
    more than its own."""
    ops = nets[1]
    ra = _dev(ops, roots, 0, 24)
    ra = (ra[0], ra[1], torch.zeros_like(ra[2]))
    fresh = _engine(nets, "a", "a", 24, 16)
    before = {k: getattr(fresh.tree, k).cpu().numpy().copy() for k in POOL}
    (ma, a), (mb, b) = _arena(nets, ra, split_24_8["rb"], 16, 16, net_workgroups=net_workgroups)
    for k in POOL:
        assert np.array_equal(a[k], before[k]), k          # A's pool: untouched, byte for byte
    assert a["policy_evals"] == 0 and a["fresh_leaves"] == 0
    _same(b, split_24_8["twin_b"], True, "B")


def test_constants_are_per_agent(nets, roots):
    """A: 16 playouts, lmbda 0.5; B: 24 playouts, lmbda 0 (no rollouts), c_puct 2."""
    ops = nets[1]
    ra, rb = _dev(ops, roots, 0, 24), _dev(ops, roots, 24, 32)
    kw_b = dict(lmbda=0.0, c_puct=2.0)
    (ma, a), (mb, b) = _arena(nets, ra, rb, 16, 24, kw_b=kw_b)
    _same(a, _alone(nets, "a", "a", ra, 16), True, "A")
    _same(b, _alone(nets, "b", "b", rb, 24, **kw_b), True, "B")
    assert b["z_log_n"].sum() == 0 and a["z_log_n"].sum() == 16 * int(ra[2].sum().item())


def test_trees_are_the_oracles(nets, roots, split_24_8):
    """The first 4 active games of each agent, rebuilt by oracle/mcts_py.MCTS on that agent's nets (the production
    kernels on one board) and the rollout results the playouts backed up: trees, Q and P bit for bit, the move, the
    visit row."""
    ops, pairs = nets[1], nets[2]
    own, opp, active = roots
    s = split_24_8
    for who, m, lo in (("a", s["ma"], 0), ("b", s["mb"], 24)):
        probe = NetProbe(ops, *pairs[who])
        zlog = s[who]["z_log"]
        on = np.nonzero(active[lo:lo + m.n_games])[0]
        for g in on[:4]:
            it = iter(zlog[:16, g])
            om = mcts_py.MCTS(probe.policy_fn, probe.value_fn, lambda st, c, it=it: int(next(it)), lmbda=0.5, c_puct=1.0,
                              n_thr=N_THR)
            want = om.get_move(state_of(own[lo + g], opp[lo + g]), 1, 16)
            assert next(it, None) is None
            _cmp_tree(m.tree.dump(int(g), max_depth=64), mcts_py.dump_tree(om.root, max_depth=64), "%s g%d" % (who, g))
            k = int(np.nonzero(on == g)[0][0])
            assert s[who]["move"][k] == (-2 if want is None else want), (who, g)
            for act, ch in om.root.children.items():
                if act >= 0:
                    assert s[who]["visits"][k, act] == ch.n_visits


def test_refusals_launch_nothing(nets, roots):
    from iago_amd import _lib
    ops = nets[1]
    ra, rb = _dev(ops, roots, 0, 24), _dev(ops, roots, 24, 32)
    ma, mb = _engine(nets, "a", "a", 24, 16), _engine(nets, "b", "b", 8, 16)
    for m in (ma, mb):
        m.reserve_net_rows(ma.resident_workgroups)
        m._ps["ctl"].fill_(77)                             # (a launch would clear it)
    codes = torch.ones(24, dtype=torch.uint8, device="cuda")
    codes[3] = 2

    def sets(active_a=ra[2]):
        a, ka = ma._search_args(ra[0], ra[1], active_a, 16)
        b, kb = mb._search_args(rb[0], rb[1], rb[2], 16)
        return a, b, (ka, kb)

    def whole_games(a, b):
        a.max_turns = 4

    def stream(a, b):
        b.games_total = 5

    def shared_ctl(a, b):
        b.ctl = a.ctl

    def shared_tree(a, b):
        b.tree = a.tree

    for change in (whole_games, stream, shared_ctl, shared_tree):
        a, b, keep = sets()
        change(a, b)
        assert ops.search_arena(a, b, check_result=False) == _lib.IAGO_ERR_INVALID, change.__name__
    a, b, keep = sets(codes)
    assert ops.search_arena(a, b, check_result=False) == _lib.IAGO_ERR_INVALID      # a match code in `active`
    a, b, keep = sets()
    assert ops.search_arena(a, None, check_result=False) == _lib.IAGO_ERR_INVALID   # a null set
    assert ops.search_arena(None, b, check_result=False) == _lib.IAGO_ERR_INVALID
    with pytest.raises(_lib.IagoError, match="iago_mcts_search_arena") as err:
        ops.search_arena(None, b)
    assert err.value.rc == _lib.IAGO_ERR_INVALID
    torch.cuda.synchronize()
    for m in (ma, mb):
        assert bool((m._ps["ctl"] == 77).all()) and int(m.tree.n_nodes.max().item()) == 1
