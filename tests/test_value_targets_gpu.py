"""The value targets on the GPU, bit for bit against tests/value_targets_ref.py: iago_mcts_root_value against the trees'
own root nodes and against the oracle's negamax trees, iago_value_targets and iago_replay_merge_values against the numpy
rules on random records, whole games with root values recorded (the record changes no game), and the replay window's
value column through plain and merged draws."""
import numpy as np
import pytest
import torch

from oracle import mcts_py
from tests import negamax_ref
from tests import value_targets_ref as ref
from tests.gpu_util import state_of
from tests.test_mcts_production_gpu import NetProbe

pytestmark = pytest.mark.gpu

Q16 = 65536
START_OWN, START_OPP = 0x0000000810000000, 0x0000001008000000
RECORDS = ("own", "opp", "move", "pi", "valid", "z")


@pytest.fixture(scope="module")
def nets():
    from iago_amd import engine, network, ops
    assert torch.cuda.is_available()
    torch.manual_seed(0)
    policy, value = network.SLPolicy().cuda().eval(), network.Value().cuda().eval()
    return engine, ops, policy, value, ops.uniform_weights()


def _engine(nets, G, n_sims=20, **kw):
    engine, ops, policy, value, rw = nets
    return engine.BatchedMCTS(G, policy, value, rw, n_thr=1, capacity=engine.suggest_capacity(n_sims, 1), seed=7,
                              game_id_base=300, persistent=True, backup="negamax", **kw)


def _roots(m):
    """(n_visits, q) of every game's root node, read from the pool."""
    at = torch.arange(m.n_games, device="cuda") * m.tree.capacity + m.tree.root.to(torch.int64)
    return m.tree.n_visits[at].cpu().numpy(), m.tree.q[at].cpu().numpy()


# ---- 1. iago_mcts_root_value
@pytest.mark.parametrize("G, inactive", [(3, (1,)), (65, tuple(range(0, 65, 3)))])
def test_root_value_is_the_roots_own_node(nets, G, inactive):
    engine, ops = nets[:2]
    m = _engine(nets, G)
    own, opp = ops.bits_to_tensor([START_OWN] * G), ops.bits_to_tensor([START_OPP] * G)
    every = torch.ones(G, dtype=torch.uint8, device="cuda")
    m.search(own, opp, every, 20)
    n_root, q_root = _roots(m)
    assert np.all(n_root == 20) and np.any(q_root != 0)
    want_q, want_flags = ref.root_value_q16(q_root, with_flags=True)
    q16, n = m.root_value()                                            # active None: every game
    assert q16.dtype == torch.int32 and n.dtype == torch.int32
    assert np.array_equal(q16.cpu().numpy(), want_q) and np.array_equal(n.cpu().numpy(), n_root)
    active = every.clone()
    active[list(inactive)] = 0
    flags = torch.zeros(1, dtype=torch.int32, device="cuda")
    q16, n = ops.mcts_root_value(m.tree.ref(), active, flags=flags)    # (fresh buffers: every entry is written)
    on = active.cpu().numpy() != 0
    assert np.array_equal(q16.cpu().numpy(), np.where(on, want_q, 0))
    assert np.array_equal(n.cpu().numpy(), np.where(on, n_root, 0))
    assert int(flags.item()) == want_flags == 0
    # planted roots: ties to even, beyond +-1, saturation, NaN -- the rule on values no search of these nets gives
    planted = np.array([0.5 * 2.0 ** -16, -2.5 * 2.0 ** -16, 3.25, -16384.0, 16385.0, np.nan, -3e38], np.float32)[:G]
    at = torch.arange(len(planted), device="cuda") * m.tree.capacity + m.tree.root[:len(planted)].to(torch.int64)
    m.tree.q[at] = torch.from_numpy(planted).cuda()
    want_q, want_flags = ref.root_value_q16(_roots(m)[1], with_flags=True)
    flags.zero_()
    q16, n = ops.mcts_root_value(m.tree.ref(), every, flags=flags)
    assert np.array_equal(q16.cpu().numpy(), want_q) and int(flags.item()) == want_flags
    assert want_flags == (ref.SATURATED | ref.NAN if G > 3 else 0)
    with pytest.raises(ValueError, match="entries"):
        ops.mcts_root_value(m.tree.ref(), every[:-1])
    m.close()


def test_root_value_against_the_oracles_negamax_tree(nets):
    """Turn 0 of 4 games: the root of oracle.mcts_py.MCTS under tests/negamax_ref.py, fed the search's own rollout
    results and the production nets on one board."""
    engine, ops, policy, value, rw = nets
    G, n_sims = 4, 20
    m = _engine(nets, G, z_log_rows=n_sims)
    own, opp = ops.bits_to_tensor([START_OWN] * G), ops.bits_to_tensor([START_OPP] * G)
    m.search(own, opp, torch.ones(G, dtype=torch.uint8, device="cuda"), n_sims)
    q16, n = (t.cpu().numpy().copy() for t in m.root_value())
    z_log = m.z_log.cpu().numpy()
    assert np.all(m.z_log_n.cpu().numpy() == n_sims)
    probe = NetProbe(ops, policy, value)
    with negamax_ref.rule():
        for g in range(G):
            it = iter(z_log[:n_sims, g])
            om = mcts_py.MCTS(probe.policy_fn, probe.value_fn, lambda s, c, it=it: int(next(it)), lmbda=0.5, c_puct=1.0,
                              n_thr=1)
            om.get_move(state_of(START_OWN, START_OPP), 1, n_sims)
            assert next(it, None) is None
            assert int(n[g]) == om.root.n_visits == n_sims, g
            assert int(q16[g]) == int(ref.root_value_q16(np.array([om.root.Q], np.float32))[0]), g
    assert len(set(q16.tolist())) > 1                                   # (the games differ: their rollouts do)
    m.close()


# ---- 2. iago_value_targets
@pytest.fixture(scope="module")
def records():
    """Random records of every shape, made once: valid over all six kinds, q over +-2^30 with the clip's edges planted."""
    rs = np.random.RandomState(5)
    out = {}
    for B in (1, 63, 64, 65, 130):
        for T in (1, 2, 7, 61):
            valid = rs.randint(0, 6, size=(T, B)).astype(np.uint8)
            q = rs.randint(-(1 << 30), (1 << 30) + 1, size=(T, B), dtype=np.int64).astype(np.int32)
            near = rs.randint(0, 3, size=(T, B))                       # a third of the rows inside the clip, a third at its edges
            q = np.where(near == 0, q % (2 * Q16 + 1) - Q16, q).astype(np.int32)
            q = np.where(near == 1, rs.choice([-(1 << 30), -Q16 - 1, -Q16, Q16, Q16 + 1, 1 << 30], size=(T, B)), q).astype(np.int32)
            score = rs.randint(-64, 65, size=(T, B)).astype(np.int8)
            z = rs.randint(-1, 2, size=B).astype(np.int8)
            mover = np.asarray([1 if t % 2 == 0 else 2 for t in range(T)], np.int8)
            out[T, B] = (valid, q, score, z, mover)
    return out


@pytest.mark.parametrize("lam, mix", [(256, 0), (0, 0), (128, 0), (243, 64), (256, 128), (0, 256)])
def test_value_targets_bit_exact(nets, records, lam, mix):
    ops = nets[1]
    for (T, B), (valid, q, score, z, mover) in records.items():
        got = ops.value_targets(*(torch.from_numpy(x).cuda() for x in (valid, q, score, z, mover)), lam, mix)
        assert got.dtype == torch.int32 and tuple(got.shape) == (T, B)
        want = ref.value_targets(valid, q, score, z, mover, lam, mix)
        assert np.array_equal(got.cpu().numpy(), want), (T, B, lam, mix)
        assert np.abs(want.astype(np.int64)).max() <= Q16
    # the mover as a sequence of colours, no score record
    valid, q, score, z, mover = records[7, 65]
    v = np.where(valid == 3, 0, valid).astype(np.uint8)
    got = ops.value_targets(torch.from_numpy(v).cuda(), torch.from_numpy(q).cuda(), None, torch.from_numpy(z).cuda(),
                            mover.tolist(), lam, mix)
    assert np.array_equal(got.cpu().numpy(), ref.value_targets(v, q, score, z, mover, lam, mix))


# ---- 3. iago_replay_merge_values
@pytest.mark.parametrize("count, sizes", [(1, [1]), (63, [1, 62]), (64, [64]), (65, [65]),
                                          (1000, [1, 64, 65, 600, 1, 3, 200, 66])])
def test_merge_values_bit_exact(nets, count, sizes):
    ops = nets[1]
    assert sum(sizes) == count
    rs = np.random.RandomState(count)
    order = rs.permutation(count).astype(np.int32)
    group = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    mult = np.asarray(sizes, np.int32)
    first = (np.cumsum(sizes) - mult).astype(np.int64)
    v = rs.choice([-(1 << 30), 1 << 30, 12345, -1], size=count + 5).astype(np.int32)   # (a column longer than the window's count)
    big = int(np.argmax(sizes))
    v[order[first[big]:first[big] + mult[big]]] = 1 << 30             # the largest group: every row at +2^30
    flags = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = ops.replay_merge_values(*(torch.from_numpy(x).cuda() for x in (order, group, first, mult, v)), flags=flags)
    want = ref.merge_values(order, group, v)
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want) and int(flags.item()) == 0
    assert count < 64 or int(want[big]) == sizes[big] << 30 > 2 ** 31
    # what the device refuses to index by: a slot outside the window and a wrong group number are left out, a span is clamped
    if count == 1000:
        from iago_amd import _lib
        o2, g2, m2 = order.copy(), group.copy(), mult.copy()
        o2[first[3] + 5], g2[first[6] + 1], m2[7] = count + 4, 0, 5000
        got = ops.replay_merge_values(*(torch.from_numpy(x).cuda() for x in (o2, g2, first, m2, v)), flags=flags)
        want = want.copy()
        want[3] -= v[order[first[3] + 5]]
        want[6] -= v[order[first[6] + 1]]
        assert np.array_equal(got.cpu().numpy(), want) and int(flags.item()) == _lib.REPLAY_MERGE_BAD_INPUT


# ---- 4. whole games
def _play(nets, **kw):
    engine = nets[0]
    m = _engine(nets, 8, n_sims=8)
    r = engine.SelfPlayEngine(m).play(8, **kw)
    m.close()
    return r


@pytest.fixture(scope="module")
def games(nets):
    return _play(nets, root_values=True)


def test_the_record_changes_no_game(nets, games):
    plain = _play(nets)
    assert plain.q is None and plain.q_visits is None and plain.launches == 1   # (whole games in one launch)
    assert games.launches == games.n_turns == plain.n_turns                      # (the turn loop)
    for k in RECORDS:
        assert torch.equal(getattr(games, k), getattr(plain, k)), k
    assert sorted(plain.tuples()) == sorted(set(games.tuples()) - {"q"})
    with pytest.raises(ValueError, match="root_values"):
        plain.tuples(value_target=(256, 0))


def test_the_recorded_values(games):
    T, B = games.valid.shape
    assert games.q.dtype == torch.int32 and tuple(games.q.shape) == tuple(games.q_visits.shape) == (T, B)
    searched = (games.valid == 1) | (games.valid == 4)
    assert int(searched.sum()) > 8 * 40
    assert not bool((games.q[~searched] != 0).any()) and not bool((games.q_visits[~searched] != 0).any())
    assert bool((games.q_visits[searched] >= 8).all())                 # (the turn's playouts, and the reused subtree's)
    assert int((games.q[searched] != 0).sum()) > int(searched.sum()) // 2
    tup = games.tuples()
    assert torch.equal(tup["q"], games.q.reshape(-1)[games.valid.reshape(-1) == 1])


def test_tuples_carry_the_targets(games):
    z = games.tuples()["z"]
    v = games.tuples(value_target=(256, 0))["v"]
    assert v.dtype == torch.int32 and torch.equal(v, Q16 * z.to(torch.int32))
    host = [games.valid.cpu().numpy(), games.q.cpu().numpy(), games.score.cpu().numpy(), games.z.cpu().numpy(), games.mover]
    want = ref.value_targets(*host, 128, 64)
    assert np.array_equal(games.value_targets(128, 64).cpu().numpy(), want)
    got = games.tuples(value_target=(128, 64))["v"].cpu().numpy()
    assert np.array_equal(got, want.reshape(-1)[host[0].reshape(-1) == 1])
    assert np.any(got != (Q16 * z.cpu().numpy().astype(np.int32)))     # (the targets are no longer the result alone)
    with pytest.raises(ValueError, match="256"):
        games.value_targets(300, 0)


def test_solved_rows_take_the_sign_of_their_score(nets):
    r = _play(nets, root_values=True, explore_turns=2, solve_empties=6)
    plain = _play(nets, explore_turns=2, solve_empties=6)
    for k in RECORDS + ("score",):
        assert torch.equal(getattr(r, k), getattr(plain, k)), k
    rows = r.solved_tuples(value_target=(0, 256))
    assert rows["v"].numel() >= 8 and torch.equal(rows["v"], Q16 * torch.sign(rows["score"]).to(torch.int32))
    assert not bool((r.q[r.valid == 3] != 0).any())
    host = [r.valid.cpu().numpy(), r.q.cpu().numpy(), r.score.cpu().numpy(), r.z.cpu().numpy(), r.mover]
    assert np.array_equal(r.value_targets(243, 64).cpu().numpy(), ref.value_targets(*host, 243, 64))


def test_a_stream_records_them_batch_by_batch(nets, games):
    """12 games through 8 slots: the batch loop, whose first batch is play()'s games."""
    engine = nets[0]
    m = _engine(nets, 8, n_sims=8)
    r = engine.SelfPlayEngine(m).play_stream(8, 12, root_values=True)
    m.close()
    T = min(r.n_turns, games.n_turns)
    assert tuple(r.q.shape) == tuple(r.q_visits.shape) == tuple(r.valid.shape) == (r.n_turns, 12) and r.launches == 2
    for k in ("valid", "move", "q", "q_visits"):
        assert torch.equal(getattr(r, k)[:T, :8], getattr(games, k)[:T]), k
    assert torch.equal(r.z[:8], games.z)
    searched = (r.valid == 1) | (r.valid == 4)
    assert not bool((r.q[~searched] != 0).any()) and bool((r.q_visits[searched] >= 8).all())
    host = [r.valid.cpu().numpy(), r.q.cpu().numpy(), r.score.cpu().numpy(), r.z.cpu().numpy(), r.mover]
    assert np.array_equal(r.value_targets(128, 64).cpu().numpy(), ref.value_targets(*host, 128, 64))


# ---- 5. the window
def test_the_window_draws_the_value_column(nets, games):
    from iago_amd.replay import ReplayWindow
    ops = nets[1]
    tup = games.tuples(value_target=(128, 64))
    rows = int(tup["own"].numel())
    w = ReplayWindow(rows, seed=3, value_targets=True)
    assert w.add(tup) == rows
    assert torch.equal(w.cols["v"], tup["v"])
    s = w.sample(16)
    assert sorted(s) == ["move", "opp", "own", "pi", "result", "slot", "sym", "v", "z"]
    assert torch.equal(s["v"], w.cols["v"][s["slot"].to(torch.int64)])
    assert s["result"].dtype == torch.float32
    assert np.array_equal(s["result"].cpu().numpy(), s["v"].cpu().numpy().astype(np.float32) / np.float32(Q16))
    u = w.sample(16, merged="unique")
    assert sorted(u) == ["group", "mult", "opp", "own", "pi", "result", "sym", "v_sum", "z_sum"]
    c = w.cols
    m = ops.replay_merge(c["own"], c["opp"], c["pi"], c["z"], w.count)
    sums = ref.merge_values(m["order"].cpu().numpy(), m["group"].cpu().numpy(), c["v"].cpu().numpy())
    merged = w.merged()
    assert merged.n_unique == len(sums) < rows                          # (eight games share their first positions)
    assert merged.v_sum.dtype == torch.int64 and np.array_equal(merged.v_sum.cpu().numpy(), sums)
    group = u["group"].cpu().numpy()
    assert np.array_equal(u["v_sum"].cpu().numpy(), sums[group])
    want = (sums[group].astype(np.float64) / (65536.0 * u["mult"].cpu().numpy().astype(np.float64))).astype(np.float32)
    assert u["result"].dtype == torch.float32 and np.array_equal(u["result"].cpu().numpy(), want)
    # a window built without value targets: the dicts of before
    old = ReplayWindow(rows, seed=3)
    old.add(tup)
    s0, u0 = old.sample(16), old.sample(16, merged="unique")
    assert sorted(s0) == ["move", "opp", "own", "pi", "result", "slot", "sym", "z"]
    assert sorted(u0) == ["group", "mult", "opp", "own", "pi", "result", "sym", "z_sum"]
    assert old.merged().v_sum is None
    for k in ("own", "opp", "pi", "move", "z", "slot", "sym"):          # the same draw: the value column changes no row
        assert torch.equal(s0[k], s[k]), k
    assert torch.equal(s0["result"], s["z"].to(torch.float32))
