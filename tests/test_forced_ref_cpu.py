"""Forced playouts and policy-target pruning on the CPU: the reference rule (tests/forced_ref.py) -- forced() and
prune_row() by their properties and on a hand-built root --, the oracle subclass the GPU tests compare with, the entry
points (declared, exported, refusing bad arguments without a device) and the engine's ValueErrors."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from oracle import mcts_py
from oracle import oracle as orc
from tests import forced_ref as fr, root_noise_ref as rn
from tests.test_search_refusals_cpu import INVALID, Call

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 11
NOISE, K256 = (77, 128), 512          # what tests/test_forced_gpu.py plays with
F32 = np.float32


# ---- forced()
def test_forced_is_the_square_root_bound_and_monotone_in_n():
    rng = np.random.default_rng(5)
    for _ in range(200):
        p = F32(rng.uniform(0.1, 1.1))
        N = int(rng.integers(0, 2000))
        k = int(rng.integers(1, 4097))
        flags = [fr.forced(n, p, N, k) for n in range(0, 80)]
        assert not flags[0]                                           # n >= 1
        first_miss = flags[1:].index(False) + 1 if False in flags[1:] else 80
        assert not any(flags[first_miss:])                            # true up to a bound, false from it on
        bound = math.sqrt(k / 256 * float(p) * N)
        assert all(abs(n - bound) < 1e-6 or flags[n] == (n < bound) for n in range(1, 80))
    assert not fr.forced(1, F32(1.1), 0, 4096)                        # a root without visits forces nothing
    assert fr.forced(1, F32(0.5), 2, 512) and not fr.forced(2, F32(0.5), 2, 512)     # 256 < 512, 1024 < 512 fails
    assert not fr.forced(1, F32(0.5), 1, 512)                         # 256 < 256 fails: strict


def test_forced_is_the_rule_in_python_floats():
    """k_256 p is exact in float64 (12 x 24 bits); its product with N is the one rounding -- what python's own floats do."""
    rng = np.random.default_rng(9)
    for _ in range(20000):
        p = F32(rng.uniform(0.1, 1.1))
        N, k, n = int(rng.integers(1, 4000)), int(rng.integers(1, 4097)), int(rng.integers(1, 60))
        assert fr.forced(n, p, N, k) == (256 * n * n < k * float(p) * N)
        assert float(k) * float(p) == k * float(p) and int(float(k) * float(p) * 2.0 ** 40) == float(k) * float(p) * 2.0 ** 40


# ---- prune_row()
def _random_root(rng, K):
    acts = sorted(rng.choice(64, size=K, replace=False).tolist())
    ns = np.where(rng.integers(0, 2, size=K) == 0, rng.integers(0, 30, size=K), rng.integers(0, 5, size=K))   # (few visits too)
    ch = [(a, int(n), F32(rng.uniform(0.1, 1.1)), F32(rng.uniform(-1, 1)) if n else 0) for a, n in zip(acts, ns)]
    return ch, int(ns.sum()) + int(rng.integers(0, 16))


def test_prune_row_properties():
    rng = np.random.default_rng(7)
    reduced = zeroed = 0
    for trial in range(400):
        ch, N = _random_root(rng, int(rng.integers(2, 20)))
        k = int(rng.choice([1, 64, 512, 4096]))
        raw = np.zeros(64, np.int64)
        for a, n, _, _ in ch:
            raw[a] = n
        row = fr.prune_row(ch, N, 1.0, k)
        assert np.all(row <= raw) and np.all(row >= 0)                # never raises a count
        assert not row[[a for a in range(64) if a not in [c[0] for c in ch]]].any()
        b = int(np.argmax(raw))
        assert row[b] == raw[b] and int(np.argmax(row)) == b          # b and the argmax stay
        less = row < raw
        assert not np.any(row[less] == 1)                             # never leaves a reduced child at 1
        reduced += int(less.sum())
        zeroed += int((less & (row == 0)).sum())
        for a, n, p, _ in ch:                                         # at most the forced visits are given back
            f = sum(fr.forced(j, p, N, k) for j in range(1, n))
            assert raw[a] - row[a] <= f or (row[a] == 0 and raw[a] - 1 <= f)
    assert reduced > 100 and zeroed > 10


def test_prune_row_returns_the_raw_row_when_nothing_is_forced():
    rng = np.random.default_rng(8)
    for _ in range(100):
        ch, N = _random_root(rng, int(rng.integers(2, 20)))
        N = min(N, 200)                                               # k_256 p N <= 1 * 1.1 * 200 < 256: forced(1) fails
        raw = np.zeros(64, np.int64)
        for a, n, _, _ in ch:
            raw[a] = n
        assert np.array_equal(fr.prune_row(ch, N, 1.0, 1), raw)
    # fewer than two children: the raw row whatever k
    assert fr.prune_row([(19, 7, F32(1.1), F32(0.5))], 8, 1.0, 4096)[19] == 7
    assert not fr.prune_row([(-1, 7, F32(1.1), F32(0.5))], 8, 1.0, 4096).any()
    assert not fr.prune_row([], 8, 1.0, 4096).any()


def test_a_hand_built_root():
    """N = 100, c_puct 1, k = 2.  b (cell 10): n 60, Q 0.5, P 0.6 -> S* = 0.5 + 0.6 * 10 / 60.01 = 0.59998...
    Cell 20: n 30, Q 0.55, P 0.3 -- PUCT alone justifies every visit: with 29 visits it scores 0.55 + 3 / 29.01 = 0.653 >
    S*, so nothing is given back although forced(j) holds for j < sqrt(2 * 0.3 * 100) = 7.7.
    Cell 30: n 4, Q -0.9, P 0.11 -- visited only by force (forced(j) for j < 4.69: F = 3): 3, 2, 1 visits score -0.9 +
    1.1 / (0.01 + m) < S* each, so m falls to 1 and then to 0.
    Cell 40: n 9, Q 0.2, P 0.5 -- forced(j) for j < 10 -> F = 8; with m - 1 visits it scores 0.2 + 5 / (0.01 + m - 1),
    below S* = 0.59998 while m - 1 > 12.49: never -> not reduced."""
    ch = [(10, 60, F32(0.6), F32(0.5)), (20, 30, F32(0.3), F32(0.55)), (30, 4, F32(0.11), F32(-0.9)),
          (40, 9, F32(0.5), F32(0.2))]
    row = fr.prune_row(ch, 100, 1.0, 512)
    assert (int(row[10]), int(row[20]), int(row[30]), int(row[40])) == (60, 30, 0, 9) and int(row.sum()) == 99
    assert [sum(fr.forced(j, c[2], 100, 512) for j in range(1, c[1])) for c in ch[1:]] == [7, 3, 8]
    # a child forced past what PUCT grants gives back exactly the visits whose score stays below S*, and stops at F:
    # cell 50: n 12, Q 0.0, P 1.0 -> forced for j < 14.1: F = 11; score with m - 1 visits = 10 / (0.01 + m - 1) < 0.59998
    # needs m - 1 > 16.66: never at n 12 -> kept.  With Q -0.5: 10 / (m - 0.99) < 1.09998 -> m - 1 >= 10 -> m 12 -> 11 -> stop
    row = fr.prune_row(ch + [(50, 12, F32(1.0), F32(-0.5))], 100, 1.0, 512)
    assert int(row[50]) == 10                    # m - 1 = 11 and 10 score 0.408 and 0.499 < S*; 9 scores 0.61: kept
    # the first maximum is b: two children tied at the top, the second one is pruned like any other
    tie = [(10, 20, F32(0.3), F32(0.0)), (20, 20, F32(0.3), F32(-0.9))]
    row = fr.prune_row(tie, 40, 1.0, 4096)
    assert int(row[10]) == 20 and int(row[20]) < 20


# ---- the oracle subclass
def _policy(x):
    x = np.asarray(x, np.float32).reshape(-1)
    h = (np.arange(64) * 37 + int(x[:64].sum()) * 11 + int(x[64:].sum()) * 5) % 64
    p = (h + 1).astype(np.float32)
    return p / p.sum()


def _value(x):            # (values and results that differ by position: with all Q equal PUCT alone spreads the visits)
    x = np.asarray(x, np.float32).reshape(-1)
    return F32((int((x[:64] * np.arange(1, 65)).sum()) * 7 + int((x[64:] * np.arange(1, 65)).sum()) * 3) % 17 / 8.0 - 1.0)


def _rollout(state, c):
    return int((np.asarray(state).reshape(-1) * np.arange(1, 65)).sum() + c) % 3 - 1


def _mcts(cls, n_thr, game_id=300, **kw):
    return cls(_policy, _value, _rollout, lmbda=0.5, c_puct=1.0, n_thr=n_thr,
               noise=NOISE + (rn.DRAWS,), seed=SEED, game_id=game_id, **kw)


def _turns(m, n_sims, turns=3):
    state, color, out = orc.initial_state(), 1, []
    for t in range(turns):
        m.begin_turn(state, color, t)
        a = m.get_move(state, color, n_sims)
        out.append((mcts_py.dump_tree(m.root, max_depth=64), fr.raw_row(m.root)))
        m.update_with_move(a)
        orc.place_stone(state, a, color)
        color = 3 - color
    return out


@pytest.mark.parametrize("n_thr,n_sims", [(15, 40), (1, 24)])
def test_with_no_forcing_active_the_subclass_is_noisy_mcts(n_thr, n_sims):
    plain = _turns(_mcts(rn.NoisyMCTS, n_thr), n_sims)
    for kw in (dict(k_256=None), dict(k_256=0)):
        got = _turns(_mcts(fr.ForcedMCTS, n_thr, **kw), n_sims)
        assert all(a[0] == b[0] for a, b in zip(got, plain))
    # a turn begun clean (a fast turn of the playout cap) is not forced either
    a, b = _mcts(fr.ForcedMCTS, n_thr, k_256=K256), _mcts(rn.NoisyMCTS, n_thr)
    state = orc.initial_state()
    for m in (a, b):
        m.begin_turn(state, 1, 0, noised=False)
        m.get_move(state, 1, n_sims)
    assert mcts_py.dump_tree(a.root, max_depth=64) == mcts_py.dump_tree(b.root, max_depth=64) and a.n_forced == 0


@pytest.mark.parametrize("n_thr,n_sims", [(15, 40), (1, 24)])
def test_forcing_moves_visits_at_the_gpu_tests_parameters(n_thr, n_sims):
    """Non-vacuity: at (alpha, eps) = (77, 128), k_256 = 512 and the GPU tests' playouts the forced search differs from
    the noised one in a root child's count, forcing never leaks below the root, and pruning takes visits back."""
    differ = pruned = 0
    for game_id in range(300, 308):
        f, n = _mcts(fr.ForcedMCTS, n_thr, game_id=game_id, k_256=K256), _mcts(rn.NoisyMCTS, n_thr, game_id=game_id)
        state, color = orc.initial_state(), 1
        for t in range(4):                       # (the same game while the two searches agree; reused roots from turn 1 on)
            for m in (f, n):
                m.begin_turn(state, color, t)
            a = f.get_move(state, color, n_sims)
            n.get_move(state, color, n_sims)
            row, raw = f.pruned_row(), fr.raw_row(f.root)
            assert np.all(row <= raw)
            pruned += int(row.sum()) < int(raw.sum())
            if not np.array_equal(raw, fr.raw_row(n.root)):
                differ += 1
                break
            for m in (f, n):
                m.update_with_move(a)
            orc.place_stone(state, a, color)
            color = 3 - color
        assert f.n_forced > 0
    print("n_thr %d: games of 8 whose root counts differ %d, whose row was pruned %d" % (n_thr, differ, pruned))
    assert differ >= 1 and pruned >= 1


def test_forcing_acts_at_the_root_only():
    """With every node's select spied on: +inf is offered at the root alone, and below the root the forced tree's
    selections are Node.select's."""
    m = _mcts(fr.ForcedMCTS, 1, k_256=4096)
    seen = []
    real = m.select

    def spy(node):
        got = real(node)
        if node is not m.root:
            assert got[0] == node.select(m.c_puct)[0]
        seen.append(node is m.root)
        return got
    m.select = spy
    state = orc.initial_state()
    m.begin_turn(state, 1, 0)
    m.get_move(state, 1, 60)
    assert any(seen) and not all(seen) and m.n_forced > 0


# ---- the entry points
def _forced_args(L, counts=0x7E0000100000, alpha=77, eps=128, draws=256, k=K256):
    z = L.SearchForcedArgs()
    z.noise.alpha_256, z.noise.eps_256, z.noise.draws, z.noise.counts = alpha, eps, draws, counts
    z.k_256 = k
    return z


def test_entry_points_are_declared_exported_and_mirrored():
    from iago_amd import _lib as L, build
    build.build()
    text = open(os.path.join(ROOT, "include", "iago_hip_serving.h")).read()
    declared = set(re.findall(r"IAGO_API[^;(]*?\b(iago_\w+)\s*\(", text))
    for name in ("iago_mcts_search_forced", "iago_mcts_prune_visits"):
        assert name in declared and name in L.SERVING_SYMBOLS and hasattr(L.lib(), name), name
    assert [f[0] for f in L.SearchForcedArgs._fields_] == ["noise", "streams", "k_256", "reserved0", "reserved"]
    assert C.sizeof(L.SearchForcedArgs) == 24 + 8 + 8 + 32
    # the noise search's struct is as it was: its reserved words are not reused
    assert [f[0] for f in L.SearchNoiseArgs._fields_] == ["noise", "streams", "reserved"]
    main = open(os.path.join(ROOT, "include", "iago_hip.h")).read()
    assert "iago_mcts_search_forced" not in main and "iago_mcts_prune_visits" not in main   # (serving's, not the core header's)


def _refused(rc_err, who, what):
    rc, err = rc_err
    assert rc == INVALID and err.startswith(who) and what in err, (rc, err)


def test_search_forced_refusals():
    from iago_amd import _lib as L
    lib = L.lib()

    def call(c, z):
        return lib.iago_mcts_search_forced(None if c is None else C.byref(c.a), None if z is None else C.byref(z), None), \
            lib.iago_last_error()
    who = b"iago_mcts_search_forced"
    one = Call("persistent")
    _refused(call(None, _forced_args(L)), who, b"null args")
    _refused(call(one, None), who, b"null args")
    # what the noise search refuses
    for fault, what in ((dict(alpha=0), b"alpha_256"), (dict(alpha=4097), b"alpha_256"), (dict(eps=-1), b"eps_256"),
                        (dict(eps=257), b"eps_256"), (dict(draws=8), b"draws"), (dict(draws=96), b"draws"),
                        (dict(counts=None), b"counts")):
        _refused(call(one, _forced_args(L, **fault)), who, what)
    z = _forced_args(L)
    z.reserved[2] = 1
    _refused(call(one, z), who, b"reserved")
    z = _forced_args(L)
    z.reserved0 = 1
    _refused(call(one, z), who, b"reserved")
    z = _forced_args(L)
    z.noise.reserved0 = 1
    _refused(call(one, z), who, b"reserved")
    _refused(call(Call("persistent", whole=True), _forced_args(L)), who, b"one search per launch")
    stream = Call("persistent", whole=True)
    stream.a.games_total = 8
    _refused(call(stream, _forced_args(L)), who, b"one search per launch")
    # its own
    for k in (0, -1, 4097, 1 << 20):
        _refused(call(one, _forced_args(L, k=k)), who, b"k_256")


def test_prune_visits_refusals():
    from iago_amd import _lib as L
    lib = L.lib()
    one = Call("persistent")
    f = 0x7E0000200000
    who = b"iago_mcts_prune_visits"

    def call(tree, k, out):
        return lib.iago_mcts_prune_visits(tree, None, 1.0, k, out, None), lib.iago_last_error()
    _refused(call(None, K256, f), who, b"bad tree")
    for k in (0, -1, 4097):
        _refused(call(C.byref(one.tree), k, f), who, b"k_256")
    _refused(call(C.byref(one.tree), K256, None), who, b"null pruned")


# ---- the engine's arguments
def test_forced_playouts_arg_and_play_rules():
    from iago_amd import engine, ops
    assert ops.forced_playouts_arg(None, None) is None and ops.forced_playouts_arg(None, (77, 64, 256)) is None
    assert ops.forced_playouts_arg(512, (77, 0, 256)) == 512 and ops.forced_playouts_arg(1, (77, 64, 256)) == 1
    for bad in (0, 4097, -3, 2.0, True, "512", (512,)):
        with pytest.raises(ValueError, match="forced_playouts"):
            ops.forced_playouts_arg(bad, (77, 64, 256))
    with pytest.raises(ValueError, match="requires root_noise"):
        ops.forced_playouts_arg(512, None)
    r = engine._play_rules(32, root_noise=(77, 0), forced_playouts=512)
    assert r.root_noise == (77, 0, 256) and r.forced_playouts == 512 and r[:3] == (None, 0, None)
    with pytest.raises(ValueError, match="requires root_noise"):
        engine._play_rules(32, forced_playouts=512)
    with pytest.raises(ValueError, match="forced_playouts"):
        engine._play_rules(32, root_noise=(77, 64), forced_playouts=5000)
    # off is today's record
    assert engine.NO_RULES.forced_playouts is None and engine.PlayRules(None, 0, None) == engine.NO_RULES
    assert engine._play_rules(32, root_noise=(77, 64)) == engine.PlayRules(None, 0, None, (77, 64, 256))
    assert engine.SelfPlayResult().pi_raw is None and engine.MatchResult().pi_raw is None


def test_matches_and_the_arena_refuse_forced_playouts():
    """Before anything else is looked at (no engine is needed to be refused)."""
    from iago_amd import engine
    with pytest.raises(ValueError, match="forced_playouts is not available"):
        engine.SelfPlayEngine.play_match(None, 24, forced_playouts=512)
    with pytest.raises(ValueError, match="forced_playouts is not available"):
        engine.ArenaEngine.play(None, 24, forced_playouts=512)
    with pytest.raises(ValueError, match="forced_playouts is not available"):
        engine.ArenaEngine.play(None, 24, forced_playouts=0)
