"""Root noise on the CPU: the reference rule (tests/root_noise_ref.py) -- the urn's books, a hand-worked case, the mix's
ends and roundings, the moments of the Dirichlet-multinomial it promises --, the oracle subclass the GPU tests compare
with, and the entry points: declared, exported, and refusing bad arguments without a device."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from oracle import mcts_py
from oracle import oracle as orc
from tests import explore_ref, playout_cap_ref, root_noise_ref as rn
from tests.test_search_refusals_cpu import INVALID, Call

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 11


# ---- the urn
def test_the_noise_key_is_its_own():
    assert rn.NOISE_KEY not in (explore_ref.EXPLORE_KEY, playout_cap_ref.CAP_KEY, 0x4D415443, 0x52504C59)
    assert rn.NOISE_KEY == int.from_bytes(b"DIRI", "big")
    # (the counter differs too: turn in word 1, the block in word 2)
    assert rn.words(SEED, 300, 5, 16)[:4] != rn.words(SEED, 300, 6, 16)[:4] != rn.words(SEED, 301, 5, 16)[:4]
    assert rn.words(SEED, 300, 5, 32)[:16] == rn.words(SEED, 300, 5, 16)


@pytest.mark.parametrize("draws", [16, 256, 1024])
def test_counts_sum_to_n_on_the_legal_set(draws):
    state = orc.initial_state()
    acts = orc.legal_actions(state, 1)
    assert len(acts) == 4
    for g in range(6):
        c = rn.counts(acts, SEED, 0xFFFFFFF0 + g, 3, 77, draws)
        assert int(c.sum()) == draws and c.min() >= 0
        assert not c[[a for a in range(64) if a not in acts]].any()
    wide = list(range(3, 64, 3))   # 21 cells
    c = rn.counts(wide, SEED, 7, 0, 4096, draws)
    assert int(c.sum()) == draws and not c[[a for a in range(64) if a not in wide]].any()


def test_fewer_than_two_moves_draw_nothing():
    assert not rn.counts([], SEED, 1, 0, 77).any()
    assert not rn.counts([19], SEED, 1, 0, 77).any()
    assert rn.counts([19, 26], SEED, 1, 0, 77).sum() == 256


def test_a_hand_worked_urn():
    """K = 2 (cells 19 and 26), alpha_256 = 256, N = 4.  Draw 0: weights (256, 256), W = 512; draw 1 after a count on 19:
    (512, 256), W = 768; and so on: a word 0 gives r = 0 -> cell 19; a word 0xFFFFFFFF gives r = W - 1 -> cell 26."""
    F = 0xFFFFFFFF
    cells = lambda c: (int(c[19]), int(c[26]))
    assert cells(rn.urn([19, 26], 256, 4, [0, 0, 0, 0])) == (4, 0)
    assert cells(rn.urn([19, 26], 256, 4, [F, F, F, F])) == (0, 4)
    assert cells(rn.urn([19, 26], 256, 4, [0, F, 0, F])) == (2, 2)
    # r = (2^31 * W) >> 32 = W / 2: 256 of 512 -> the second cell (256 > 256 fails); then (256, 512) of 768: r = 384 ->
    # the second again (256 > 384 fails, 768 > 384); then (256, 768) of 1024: r = 512 -> second; (256, 1024), r = 640 -> second
    assert cells(rn.urn([19, 26], 256, 4, [1 << 31] * 4)) == (0, 4)
    # alpha_256 = 1: after the first draw the drawn cell weighs 257 of 258
    assert cells(rn.urn([19, 26], 1, 4, [0, 1 << 31, 1 << 31, 1 << 31])) == (4, 0)


# ---- the mix
def test_the_mix_has_exact_ends_and_two_roundings():
    rng = np.random.default_rng(5)
    ps = (rng.random(2000, dtype=np.float32) + np.float32(0.1)).astype(np.float32)
    cs = rng.integers(0, 257, 2000)
    for p, c in zip(ps[:200], cs[:200]):
        assert rn.mix(p, c, 0).tobytes() == np.float32(p).tobytes()                      # eps 0: p, bit for bit
        assert rn.mix(p, c, 256) == np.float32(c / 256) and float(rn.mix(p, c, 256)) == c / 256   # eps 1: the share
    for draws in (16, 256, 1024):
        for eps in (1, 64, 77, 255):
            for p, c in zip(ps, cs % (draws + 1)):
                keep, term = (256 - eps) / 256, eps * int(c) / (256 * draws)
                want = np.float32(float(np.float32(float(p) * keep)) + term)             # float64, rounded twice
                assert rn.mix(p, c, eps, draws).tobytes() == want.tobytes(), (p, c, eps, draws)
    assert rn.mix(np.float32(1.1), 0, 64) == np.float32(np.float32(1.1) * np.float32(0.75))


# ---- the distribution
def test_the_counts_have_the_dirichlet_multinomial_moments():
    """M = 4096 keys at K = 8, alpha_256 = 77, N = 256: mean N / K = 32 per cell, variance N p (1 - p) (N + A) / (1 + A)
    with p = 1 / K and A = K alpha = 2.40625: 2124.1, so the standard error of a mean is 0.72."""
    M, K, alpha, N = 4096, 8, 77, 256
    cells = [2, 9, 17, 20, 33, 41, 50, 63]
    w = np.array([rn.words(SEED, g, 0, N) for g in range(M)], dtype=np.uint64)     # (M, N)
    c = np.zeros((M, K), np.int64)
    rows = np.arange(M)
    for j in range(N):
        r = (w[:, j] * np.uint64(K * alpha + 256 * j)) >> np.uint64(32)
        cum = np.cumsum(alpha + 256 * c, axis=1)
        c[rows, (cum > r.astype(np.int64)[:, None]).argmax(axis=1)] += 1
    for g in (0, 1, 4095):                                                          # (the vector form is the rule)
        assert np.array_equal(rn.counts(cells, SEED, g, 0, alpha, N)[cells], c[g])
    assert np.all(c.sum(axis=1) == N)
    A, p = K * alpha / 256, 1 / K
    var = N * p * (1 - p) * (N + A) / (1 + A)
    se = math.sqrt(var / M)
    assert abs(var - 2124.1) < 0.05 and abs(se - 0.72) < 0.005
    mean, svar = c.mean(axis=0), c.var(axis=0, ddof=1)
    print("means", np.round(mean, 2), "in standard errors", np.round((mean - N / K) / se, 2))
    print("variances", np.round(svar, 1), "ratio", np.round(svar / var, 3))
    assert np.all(np.abs(mean - N / K) <= 5 * se)
    assert np.all(np.abs(svar / var - 1) <= 0.25)


# ---- the oracle subclass
def _policy(x):
    x = np.asarray(x, np.float32).reshape(-1)
    h = (np.arange(64) * 37 + int(x[:64].sum()) * 11 + int(x[64:].sum()) * 5) % 64
    p = (h + 1).astype(np.float32)
    return p / p.sum()


def _check_tree(node, state, color, counts_of_root, eps, draws, path="root"):
    """Every child's P is Node(prob).P of its parent's position -- mixed under the root (counts given), clean elsewhere."""
    acts = orc.legal_actions(state, color)
    if not node.children:
        return 0
    n = 0
    if len(acts) < 2:
        assert len(node.children) == 1
        (a, ch), = node.children.items()
        assert a == (acts[0] if acts else -1) and ch.P == mcts_py.Node(None, 1).P, path
    else:
        prob = _policy(orc.make_state_var(state, color))
        assert list(node.children) == acts
        for a, ch in node.children.items():
            clean = mcts_py.Node(None, prob[a]).P
            want = clean if counts_of_root is None else rn.mix(clean, counts_of_root[a], eps, draws)
            assert ch.P.tobytes() == np.float32(want).tobytes(), (path, a)
            n += counts_of_root is not None
    for a, ch in node.children.items():
        s2 = orc.place_stone(np.array(state, dtype=np.float32), a, color)
        n += _check_tree(ch, s2, 3 - color, None, eps, draws, path + "/%d" % a)
    return n


@pytest.mark.parametrize("n_thr,n_sims", [(15, 24), (1, 24)])
def test_the_oracle_subclass_mixes_the_roots_children_and_nothing_else(n_thr, n_sims):
    noise = (77, 64, 64)
    m = rn.NoisyMCTS(_policy, lambda x: np.float32(0.25), lambda s, c: 0, lmbda=0.5, c_puct=1.0, n_thr=n_thr,
                     noise=noise, seed=SEED, game_id=0xFFFFFFF3)
    state, color = orc.initial_state(), 1
    seen_start, seen_expand = 0, 0
    for turn in range(4):
        acts = orc.legal_actions(state, color)
        had_children = len(m.root.children) >= 2
        before = len(m.mixed)
        m.begin_turn(state, color, turn)
        want = rn.counts(acts, SEED, 0xFFFFFFF3, turn, 77, 64)
        assert np.array_equal(m.counts, want) and int(want.sum()) == 64
        assert (len(m.mixed) - before == len(acts)) == had_children
        a = m.get_move(state, color, n_sims)
        assert len(m.mixed) - before == len(acts)                     # once per turn: at the start or in the expansion
        seen_start += had_children
        seen_expand += not had_children
        mixed = _check_tree(m.root, np.array(state, dtype=np.float32), color, want, noise[1], noise[2])
        assert mixed == len(acts)
        assert any(want[b] > 0 and ch.P != mcts_py.Node(None, _policy(orc.make_state_var(state, color))[b]).P
                   for b, ch in m.root.children.items())
        m.update_with_move(a)
        orc.place_stone(state, a, color)
        color = 3 - color
    assert seen_expand >= 1 and (n_thr == 15 or seen_start >= 1)


def test_a_clean_turn_and_eps_0_leave_the_oracles_tree():
    def tree(cls, **kw):
        m = cls(_policy, lambda x: np.float32(0.25), lambda s, c: 0, lmbda=0.5, c_puct=1.0, n_thr=3, **kw)
        state = orc.initial_state()
        if kw:
            m.begin_turn(state, 1, 0, noised=kw["noise"][1] != 64)
        m.get_move(state, 1, 20)
        return mcts_py.dump_tree(m.root)
    plain = tree(mcts_py.MCTS)
    assert tree(rn.NoisyMCTS, noise=(77, 0, 256), seed=SEED, game_id=5) == plain       # eps 0
    assert tree(rn.NoisyMCTS, noise=(77, 64, 256), seed=SEED, game_id=5) == plain      # (begin_turn(noised=False))
    assert tree(rn.NoisyMCTS, noise=(77, 65, 256), seed=SEED, game_id=5) != plain


# ---- the entry points
def _noise_args(L, counts=0x7E0000100000, alpha=77, eps=64, draws=256):
    z = L.SearchNoiseArgs()
    z.noise.alpha_256, z.noise.eps_256, z.noise.draws, z.noise.counts = alpha, eps, draws, counts
    return z


def test_entry_points_are_declared_exported_and_mirrored():
    from iago_amd import _lib as L, build
    build.build()
    text = open(os.path.join(ROOT, "include", "iago_hip_serving.h")).read()
    declared = set(re.findall(r"IAGO_API[^;(]*?\b(iago_\w+)\s*\(", text))
    for name in ("iago_mcts_root_noise", "iago_mcts_search_noise"):
        assert name in declared and name in L.SERVING_SYMBOLS and hasattr(L.lib(), name), name
    assert re.search(r"#define\s+IAGO_NOISE_KEY\s+0x44495249u", text) and L.NOISE_KEY == rn.NOISE_KEY
    assert L.NOISE_SEED_XOR == rn.NOISE_KEY << 32 and L.NOISE_DRAWS == rn.DRAWS
    assert [f[0] for f in L.RootNoise._fields_] == ["alpha_256", "eps_256", "draws", "reserved0", "counts"]
    assert C.sizeof(L.RootNoise) == 24
    assert [f[0] for f in L.SearchNoiseArgs._fields_] == ["noise", "streams", "reserved"]
    assert C.sizeof(L.SearchNoiseArgs) == 24 + 8 + 32
    assert "no longer a prefix" in " ".join(text.split()).lower()


def _refused(rc_err, who, what):
    rc, err = rc_err
    assert rc == INVALID and err.startswith(who) and what in err, (rc, err)


@pytest.mark.parametrize("fault,what", [
    (dict(alpha=0), b"alpha_256"), (dict(alpha=4097), b"alpha_256"), (dict(eps=-1), b"eps_256"), (dict(eps=257), b"eps_256"),
    (dict(draws=8), b"draws"), (dict(draws=2048), b"draws"), (dict(draws=96), b"draws"), (dict(draws=0), b"draws"),
    (dict(counts=None), b"counts"),
])
def test_both_entry_points_refuse_bad_noise(fault, what):
    from iago_amd import _lib as L
    lib = L.lib()
    c = Call("persistent")
    z = _noise_args(L, **fault)
    _refused((lib.iago_mcts_search_noise(C.byref(c.a), C.byref(z), None), lib.iago_last_error()), b"iago_mcts_search_noise", what)
    f = 0x7E0000200000
    _refused((lib.iago_mcts_root_noise(C.byref(c.tree), None, f, f, SEED, f, f, C.byref(z.noise), None), lib.iago_last_error()),
             b"iago_mcts_root_noise", what)


def test_search_noise_refusals():
    from iago_amd import _lib as L
    lib = L.lib()

    def call(c, z):
        return lib.iago_mcts_search_noise(None if c is None else C.byref(c.a), None if z is None else C.byref(z), None), \
            lib.iago_last_error()
    who = b"iago_mcts_search_noise"
    one = Call("persistent")
    _refused(call(None, _noise_args(L)), who, b"null args")
    _refused(call(one, None), who, b"null args")
    z = _noise_args(L)
    z.reserved[3] = 1
    _refused(call(one, z), who, b"reserved")
    z = _noise_args(L)
    z.noise.reserved0 = 1
    _refused(call(one, z), who, b"reserved")
    # one search per launch: whole games and streams run turn by turn
    _refused(call(Call("persistent", whole=True), _noise_args(L)), who, b"one search per launch")
    stream = Call("persistent", whole=True)
    stream.a.games_total = 8
    _refused(call(stream, _noise_args(L)), who, b"one search per launch")
    # root_noise's own
    f = 0x7E0000200000
    z = _noise_args(L)
    assert lib.iago_mcts_root_noise(None, None, f, f, SEED, f, f, C.byref(z.noise), None) == INVALID
    for args in ((None, f, f, f), (f, None, f, f), (f, f, None, f), (f, f, f, None)):
        rc = lib.iago_mcts_root_noise(C.byref(one.tree), None, args[0], args[1], SEED, args[2], args[3], C.byref(z.noise), None)
        assert rc == INVALID and lib.iago_last_error().startswith(b"iago_mcts_root_noise")
    assert lib.iago_mcts_root_noise(C.byref(one.tree), None, f, f, SEED, f, f, None, None) == INVALID


def test_the_wave_search_and_the_arena_take_no_noise():
    """Neither has a noise argument: iago_search_wave_args and iago_mcts_search_arena are as they were, and
    iago_mcts_search_noise has no wave or second set to give."""
    from iago_amd import _lib as L
    assert [f[0] for f in L.SearchWaveArgs._fields_] == ["width", "vloss", "timing", "reserved"]
    assert not any("wave" in f[0] or "arena" in f[0] for f in L.SearchNoiseArgs._fields_)
    assert len(L.lib().iago_mcts_search_arena.argtypes) == 3


def test_root_noise_arg():
    from iago_amd import engine, ops
    assert ops.root_noise_arg(None) is None
    assert ops.root_noise_arg((77, 64)) == (77, 64, 256) and ops.root_noise_arg([4096, 0, 16]) == (4096, 0, 16)
    for bad in ((0, 64), (4097, 64), (77, -1), (77, 257), (77, 64, 8), (77, 64, 96), (77, 64, 2048), (77,), 77, (77.0, 64),
                (True, 64), "ab", (77, 64, 256, 1)):
        with pytest.raises(ValueError, match="root_noise"):
            ops.root_noise_arg(bad)
    r = engine._play_rules(32, root_noise=(77, 64))
    assert r.root_noise == (77, 64, 256) and r[:3] == (None, 0, None)
    assert engine.NO_RULES.root_noise is None and engine.PlayRules(None, 0, None) == engine.NO_RULES
