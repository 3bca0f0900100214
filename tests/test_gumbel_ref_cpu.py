"""The Gumbel root search on the CPU: the reference rule (tests/gumbel_ref.py) -- the schedule, the selection order on a
hand-built root, logit_q16 against ln p on the shipped policy's golden outputs, the draw, the target -- against
ops.gumbel_schedule / ops.gumbel_tables / engine.gumbel_targets (torch float64, here on the CPU), the oracle subclass the
GPU tests compare with, the entry points (declared, exported, refusing bad arguments without a device) and the engine's
ValueErrors.

logit_q16's bound, derived: the table has 4096 buckets over the mantissa, so |logit_q16 / 65536 - ln p| <= 2^-13 (half a
bucket, d ln(1 + x) / dx <= 1) + 2^-17 (the entries' rounding) + |e - 127| * 1.43e-6 (45426 for 65536 ln 2 = 45426.094):
asserted for every normal float32 output.  It stays below 2^-12 while |e - 127| <= 64, which is asserted for every output p
>= 2^-64.  That is an ABSOLUTE bound on the logarithm, a RELATIVE bound of 2^-12 on p itself.  Relative to ln p it cannot
hold where ln p is near 0 (a lone child's p == 1.0 has logit_q16 = 8 by the rule's own formula); it is asserted as well
wherever |ln p| >= 1 and p >= 2^-64, where the absolute bound implies it.  Measured on the 16384 golden outputs: 698 are
denormal or 0 in float32 (the formula reads their bits as they are; such a move's logit is below -87 either way), the
largest error of the 15686 normal ones is 2.91e-4 at e - 127 = -126, of the 6699 with p >= 2^-64 it is 2.04e-4."""
import ctypes as C
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from oracle import mcts_py
from oracle import oracle as orc
from tests import gumbel_ref as gr, negamax_ref, selection_ref
from tests.test_search_refusals_cpu import INVALID, Call

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
F32 = np.float32
SEED = 11


@pytest.fixture(scope="module")
def tables():
    from iago_amd import ops
    return ops.gumbel_tables()


# ---- the tables and the schedule
def test_tables_are_the_formulas(tables):
    g, ln = tables
    assert g.dtype == ln.dtype == np.int32 and g.shape == (65536,) and ln.shape == (4096,)
    for u in (0, 1, 255, 32767, 32768, 65534, 65535):
        assert int(g[u]) == int(round(65536 * -math.log(-math.log((u + 0.5) / 65536)))), u
    for i in (0, 1, 7, 2047, 2048, 4095):
        assert int(ln[i]) == int(round(65536 * math.log(1 + (i + 0.5) / 4096))), i
    assert np.all(np.diff(g) > 0) and np.all(np.diff(ln) > 0)          # both strictly increasing
    assert gr.LN2_Q16 == int(round(65536 * math.log(2))) == 45426
    assert not g.flags.writeable and not ln.flags.writeable


def test_schedule_rows():
    from iago_amd import ops
    assert gr.schedule_row(4, 16) == [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5]
    assert gr.schedule_row(2, 9) == [0, 0, 1, 1, 2, 2, 3, 3, 4]
    assert gr.schedule_row(1, 5) == gr.schedule_row(0, 5) == [0, 1, 2, 3, 4]
    # non-powers of two, and a budget shorter than one round
    assert gr.schedule_row(16, 16) == [0] * 16
    assert gr.schedule_row(5, 7) == [0, 0, 0, 0, 0, 1, 1]
    assert gr.schedule_row(5, 16) == [0] * 5 + [1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6]     # L = 3: extra 1 at 5, 16 // 6 = 2 at 2
    assert gr.schedule_row(3, 12) == [0, 0, 0, 1, 1, 1] + [2, 2, 3, 3, 4, 4]         # L = 2: extra 2 at 3, 3 at 2
    for m, n in ((4, 16), (16, 16), (16, 37), (8, 5), (64, 100), (2, 1)):
        want = gr.schedule(m, n)
        got = ops.gumbel_schedule(m, n)
        assert got.dtype == np.int16 and got.shape == (m + 1, n) and np.array_equal(got, want), (m, n)
        for k in range(2, m + 1):       # a row serves counts in order: never decreasing by more than the halving allows
            row = want[k].tolist()
            assert row[0] == 0 and max(row) <= n and all(b - a in (0, 1) for a, b in zip(row, row[1:])), (m, n, k)
    for bad in ((0, 16), (65, 16), (4, 0), (4, 32768)):
        with pytest.raises(ValueError, match="gumbel_schedule"):
            ops.gumbel_schedule(*bad)


def test_a_hand_built_root_of_four_children(tables):
    """k = 4, n = 16, g = 0: every child once in the order of the priors (logit alone: all unvisited, q16 = 0), the four
    again in the order of the score (sigma's 52 * q16 dwarfs the logits' differences: the order of Q), then the best two
    by score alternately, the better first."""
    ln = tables[1]
    g = np.zeros(64, np.int64)
    acts, P, Q = [10, 20, 30, 40], [F32(0.4), F32(0.3), F32(0.2), F32(0.1)], [F32(0.1), F32(0.5), F32(-0.2), F32(0.3)]
    n = [0, 0, 0, 0]
    sched = gr.schedule(4, 16)
    seq = []
    for _ in range(16):
        ch = [(acts[i], n[i], P[i], Q[i] if n[i] else 0) for i in range(4)]
        i = gr.select(ch, g, ln, sched, 4, 16, 50, 256)
        seq.append(acts[i])
        n[i] += 1
    assert seq == [10, 20, 30, 40] + [20, 40, 10, 30] + [20, 40] * 4
    assert n == [2, 6, 2, 6]
    ch = [(acts[i], n[i], P[i], Q[i]) for i in range(4)]
    assert gr.move(ch, g, ln, 50, 256) == 20                      # the survivor: the better of the two most visited
    # the draw decides among the unvisited: a large g on the last prior brings it to the front
    g2 = g.copy()
    g2[40] = 1 << 20
    assert gr.select([(a, 0, p, 0) for a, p in zip(acts, P)], g2, ln, sched, 4, 16, 50, 256) == 3
    # m below K: only the top m by g + logit are ever visited
    n = [0, 0, 0, 0]
    sched2 = gr.schedule(2, 16)
    for _ in range(16):
        ch = [(acts[i], n[i], P[i], Q[i] if n[i] else 0) for i in range(4)]
        n[gr.select(ch, g, ln, sched2, 2, 16, 50, 256)] += 1
    assert n == [8, 8, 0, 0]
    # no child has the schedule's count (a root that was not fresh): the children of the largest count are scored
    ch = [(10, 7, P[0], Q[0]), (20, 7, P[1], Q[1]), (30, 3, P[2], Q[2])]
    assert gr.select(ch, g, ln, gr.schedule(4, 16), 4, 16, 50, 256) == 1
    # one child, a pass, no children
    assert gr.move([(19, 16, F32(1.0), F32(0.2))], g, ln, 50, 256) == 19
    assert gr.move([(-1, 16, F32(1.0), F32(0.2))], g, ln, 50, 256) == -1 and gr.move([], g, ln, 50, 256) == -2


def test_q16_and_score_are_integers():
    assert gr.q16(F32(-1.0), 3) == 0 and gr.q16(F32(1.0), 3) == 65536 and gr.q16(F32(0.0), 3) == 32768
    assert gr.q16(F32(0.7), 0) == 0                                    # unvisited
    assert gr.q16(F32(1.5 / 32768), 1) == 32768 + 2 and gr.q16(F32(2.5 / 32768), 1) == 32768 + 2   # ties to even
    assert gr.score(-5, 7, 65536, 4096, 4096, 4096) == 2 + ((8192 * 4096 * 65536) >> 8) < 1 << 53
    assert gr.score(10, -20, 100, 6, 50, 256) == -10 + 56 * 100


# ---- logit_q16 against ln p on the shipped policy's golden outputs
def test_logit_q16_on_the_shipped_policys_outputs(tables):
    ln = tables[1]
    probs = np.load(os.path.join(GOLDEN, "nets_shipped.npz"))["sl_probs"].astype(np.float32).reshape(-1)
    assert probs.size == 256 * 64
    probs = probs[probs >= F32(2.0 ** -126)]                           # the normal float32 outputs
    got = np.array([gr.logit_q16(p, ln) for p in probs], np.float64) / 65536.0
    want = np.log(probs.astype(np.float64))
    err = np.abs(got - want)
    ex = ((probs.view(np.uint32) >> 23) & 0xFF).astype(np.int64) - 127
    bound = 2.0 ** -13 + 2.0 ** -17 + np.abs(ex) * abs(45426 - 65536 * math.log(2)) / 65536
    near = ex >= -64
    print("logit_q16: %d normal outputs, max error %.3g; %d with p >= 2^-64, max error %.3g (2^-12 = %.3g)"
          % (probs.size, err.max(), near.sum(), err[near].max(), 2.0 ** -12))
    assert probs.size == 256 * 64 - 698 and np.all(err <= bound)      # (698 outputs are denormal or 0 in float32)
    assert near.sum() > 6000 and err[near].max() <= 2.0 ** -12          # a relative 2^-12 on p
    far = near & (np.abs(want) >= 1.0)
    assert far.sum() > 1000 and np.all(err[far] <= 2.0 ** -12 * np.abs(want[far]))
    assert gr.logit_q16(F32(1.0), ln) == int(ln[0]) == 8               # a lone child's p == 1.0: the same formula
    assert gr.logit_q16(F32(0.5), ln) == 8 - 45426 and gr.logit_q16(F32(0.75), ln) == int(ln[2048]) - 45426


# ---- the draw
def test_every_draw_lies_in_the_table(tables):
    g = gr.draw(SEED, 300, 0, tables[0])
    assert g.shape == (64,) and np.all(np.isin(g, tables[0]))
    key = (SEED ^ (gr.GUMBEL_KEY << 32)) & 0xFFFFFFFFFFFFFFFF
    for a in (0, 17, 63):
        assert g[a] == tables[0][int(orc.philox(key, 300, 0, a, 0)[0]) >> 16]
    # a key of its own, and every coordinate matters
    others = [gr.draw(SEED, 301, 0, tables[0]), gr.draw(SEED, 300, 1, tables[0]), gr.draw(SEED + 1, 300, 0, tables[0])]
    assert all(not np.array_equal(g, o) for o in others)
    from iago_amd import _lib
    assert _lib.GUMBEL_KEY == gr.GUMBEL_KEY and _lib.GUMBEL_SEED_XOR == gr.GUMBEL_KEY << 32
    assert len({_lib.GUMBEL_KEY, _lib.EXPLORE_KEY, _lib.CAP_KEY, _lib.NOISE_KEY, _lib.MATCH_KEY, _lib.OPENING_KEY}) == 6
    many = np.concatenate([gr.draw(SEED, 300 + k, 0, tables[0]) for k in range(40)]) / 65536.0
    assert abs(many.mean() - 0.5772) < 0.1 and abs(many.std() - 1.2825) < 0.1     # Gumbel(0, 1): Euler's constant, pi / sqrt 6


# ---- the target
def _random_rows(rng, B, tables):
    n, q, lg = np.zeros((B, 64), np.int64), np.zeros((B, 64), np.float32), np.full((B, 64), gr.INT32_MIN, np.int64)
    for b in range(B):
        K = int(rng.integers(0, 20)) if b >= 4 else (0, 1, 2, 12)[b]
        acts = sorted(rng.choice(64, size=K, replace=False).tolist())
        p = rng.dirichlet(np.full(K, 0.3)) if K else []
        for a, pa in zip(acts, p):
            lg[b, a] = gr.logit_q16(F32(max(pa, 1e-30)), tables[1])
            if b != 3 and rng.integers(0, 3) > 0:                      # (row 3: nothing visited)
                n[b, a] = int(rng.integers(1, 12))
                q[b, a] = F32(rng.uniform(-1, 1))
    return n, q, lg


def test_the_target_against_the_torch_evaluation(tables):
    from iago_amd import engine
    rng = np.random.default_rng(3)
    n, q, lg = _random_rows(rng, 400, tables)
    for c_visit, c_scale in ((50, 256), (0, 1), (4096, 64)):
        want, clear = gr.targets(n, q, lg, c_visit, c_scale)
        got = engine.gumbel_targets((torch.from_numpy(n.astype(np.int32)), torch.from_numpy(q),
                                     torch.from_numpy(lg.astype(np.int32))), c_visit, c_scale).numpy()
        assert got.dtype == np.int32 and got.shape == (400, 64)
        legal = lg != gr.INT32_MIN
        assert not got[~legal].any() and not want[~legal].any()         # zero off the legal moves
        k = legal.sum(axis=1)
        assert np.all(np.abs(got.sum(axis=1) - 65536 * (k > 0)) <= k)   # sums to scale within the legal-move count
        assert np.all(np.abs(want.sum(axis=1) - 65536 * (k > 0)) <= k)
        assert np.abs(got.astype(np.int64) - want).max() <= 1           # two correct roundings of values a few ulps apart
        assert np.array_equal(got[clear], want[clear])                  # exact away from the rounding boundaries
        print("c_visit %d c_scale_256 %d: share of clear rows %.4f" % (c_visit, c_scale, clear.mean()))
        assert clear.mean() >= 0.9
    # a root with no visited child keeps its prior; one legal move takes everything
    want, _ = gr.targets(n[3], q[3], lg[3])
    p = np.where(lg[3] != gr.INT32_MIN, np.exp(lg[3] / 65536.0), 0.0)
    assert np.array_equal(want[0], np.rint(65536 * p / p.sum()).astype(np.int64))
    assert gr.targets(n[1], q[1], lg[1])[0].max() == 65536 and not gr.targets(n[0], q[0], lg[0])[0].any()
    # another scale, and leading dimensions of any shape
    t3 = engine.gumbel_targets(tuple(torch.from_numpy(x).reshape(20, 20, 64) for x in
                                     (n.astype(np.int32), q, lg.astype(np.int32))), scale=1000).numpy()
    assert t3.shape == (20, 20, 64) and np.abs(t3.reshape(400, 64) - gr.targets(n, q, lg, scale=1000)[0]).max() <= 1
    # sigma moves mass toward the better move: two equal priors, the better q gets the larger share
    two = gr.targets([0] * 10 + [3, 3] + [0] * 52, [0] * 10 + [0.5, -0.5] + [0] * 52,
                     [gr.INT32_MIN] * 10 + [-45426, -45426] + [gr.INT32_MIN] * 52, c_visit=0, c_scale_256=16)[0][0]
    assert two[10] > two[11] > 0 and two.sum() in (65535, 65536, 65537)


# ---- the oracle subclass
def _mcts(n_thr, gumbel, tables, game_id=300):
    rng = np.random.default_rng(12)
    table = {}

    def policy(x):
        k = np.asarray(x).tobytes()
        if k not in table:
            e = np.exp(rng.normal(size=64) * 1.5)
            table[k] = (e / e.sum()).astype(np.float32)
        return table[k]

    def value(x):
        return np.float32(np.tanh(np.frombuffer(np.asarray(x, np.float32).tobytes(), np.uint8).astype(np.int64).sum() % 17 / 8.0 - 1.0))
    z = iter(np.random.default_rng(5).integers(-1, 2, size=100000).tolist())
    return gr.GumbelMCTS(policy, value, lambda s, c: next(z), lmbda=0.5, c_puct=1.0, n_thr=n_thr, gumbel=gumbel,
                         tables=tables, seed=SEED, game_id=game_id)


@pytest.mark.parametrize("n_sims,m", [(16, 4), (37, 16), (5, 8)])
def test_the_oracle_subclass_serves_the_schedule(tables, n_sims, m):
    with negamax_ref.rule(), selection_ref.rule():
        om = _mcts(1, (m, 256, 50), tables)
        state = orc.initial_state()
        om.begin_turn(0)
        mv = om.get_move(state, 1, n_sims)
        K = len(om.root.children)
        assert K == 4 and om.fallbacks == 0 and len(om.picks) == n_sims - 1     # (n_thr 1: the first playout expands nothing)
        raw = om.raw_row()
        k = min(m, K)
        # the visits are the schedule's: playout i serves a child that had sched[k][i] visits
        n = {a: 0 for a in om.root.children}
        for i, a in enumerate(om.picks):
            assert n[a] == gr.schedule_row(k, n_sims)[i], (i, a)
            n[a] += 1
        assert [n[a] for a in sorted(n)] == [int(raw[a]) for a in sorted(n)]
        assert raw[mv] == raw.max()
        # the priors are the policy's (no + 0.1), the root's children's Q the root mover's value
        rn, rq, rl = om.rows()
        assert np.array_equal(rn, raw) and np.all(rl[raw > 0] != gr.INT32_MIN) and (rl != gr.INT32_MIN).sum() == K
        assert all(ch.P.dtype == np.float32 and 0 < ch.P < 1 for ch in om.root.children.values())
        # a second turn starts from a fresh root; a plain turn (on=False) keeps the tree and plays the most visited child
        om.update_with_move(mv)
        orc.place_stone(state, mv, 1)
        om.begin_turn(1)
        assert om.root.n_visits == 0 and not om.root.children
        mv2 = om.get_move(state, 2, n_sims)
        om.update_with_move(mv2)
        orc.place_stone(state, mv2, 2)
        kept = om.root.n_visits
        om.begin_turn(2, on=False)
        assert om.root.n_visits == kept
        om.get_move(state, 1, 8)
        assert om.root.n_visits == kept + 8


# ---- the entry points
def test_entry_points_are_declared_exported_and_mirrored():
    from iago_amd import _lib as L, build
    build.build()
    text = open(os.path.join(ROOT, "include", "iago_hip_serving.h")).read()
    declared = set(re.findall(r"IAGO_API[^;(]*?\b(iago_\w+)\s*\(", text))
    for name in ("iago_mcts_gumbel_draw", "iago_mcts_search_gumbel", "iago_mcts_gumbel_finish"):
        assert name in declared and name in L.SERVING_SYMBOLS and hasattr(L.lib(), name), name
    assert [f[0] for f in L.GumbelRoot._fields_] == ["gumbel_q16", "ln_q16", "sched", "g", "m", "c_scale_256", "c_visit",
                                                     "reserved0"]
    assert C.sizeof(L.GumbelRoot) == 48 and C.sizeof(L.SearchGumbelArgs) == 48 + 8 + 32
    assert "IAGO_GUMBEL_KEY 0x%Xu" % L.GUMBEL_KEY in text
    assert L.lib().iago_abi_version() == 13


def _gumbel_args(L, m=16, c_scale=256, c_visit=50, **ptr):
    z = L.SearchGumbelArgs()
    z.gumbel.m, z.gumbel.c_scale_256, z.gumbel.c_visit = m, c_scale, c_visit
    for i, name in enumerate(("gumbel_q16", "ln_q16", "sched", "g")):
        setattr(z.gumbel, name, ptr.get(name, 0x7E0000100000 + 0x1000 * i))
    return z


def _call_ready(L, **kw):
    c = Call("persistent", **kw)
    c.a.games_per_workgroup = 32 | L.SEARCH_NEGAMAX | L.SEARCH_PUCT_AZ
    return c


def _refused(rc_err, who, what):
    rc, err = rc_err
    assert rc == INVALID and err.startswith(who) and what in err, (rc, err)


def test_search_gumbel_refusals():
    from iago_amd import _lib as L
    lib = L.lib()

    def call(c, z):
        return lib.iago_mcts_search_gumbel(None if c is None else C.byref(c.a), None if z is None else C.byref(z), None), \
            lib.iago_last_error()
    who = b"iago_mcts_search_gumbel"
    one = _call_ready(L)
    _refused(call(None, _gumbel_args(L)), who, b"null args")
    _refused(call(one, None), who, b"null args")
    for fault, what in ((dict(m=1), b"m must be"), (dict(m=65), b"m must be"), (dict(c_scale=0), b"c_scale_256"),
                        (dict(c_scale=4097), b"c_scale_256"), (dict(c_visit=-1), b"c_visit"), (dict(c_visit=4097), b"c_visit"),
                        (dict(gumbel_q16=None), b"null table"), (dict(ln_q16=None), b"null table"), (dict(g=None), b"null table"),
                        (dict(sched=None), b"null schedule")):
        _refused(call(one, _gumbel_args(L, **fault)), who, what)
    z = _gumbel_args(L)
    z.reserved[1] = 1
    _refused(call(one, z), who, b"reserved")
    z = _gumbel_args(L)
    z.gumbel.reserved0 = 1
    _refused(call(one, z), who, b"reserved")
    _refused(call(_call_ready(L, whole=True), _gumbel_args(L)), who, b"one search per launch")
    stream = _call_ready(L, whole=True)
    stream.a.games_total = 8
    _refused(call(stream, _gumbel_args(L)), who, b"one search per launch")
    for n_sims in (0, 32768):
        c = _call_ready(L)
        c.a.n_sims = n_sims
        _refused(call(c, _gumbel_args(L)), who, b"n_sims")
    # the wrong backup or selection rule
    for flags, what in ((32 | L.SEARCH_PUCT_AZ, b"negamax"), (0, b"negamax"), (32 | L.SEARCH_NEGAMAX, b"AlphaZero")):
        c = _call_ready(L)
        c.a.games_per_workgroup = flags
        _refused(call(c, _gumbel_args(L)), who, what)


def test_draw_and_finish_refusals():
    from iago_amd import _lib as L
    lib = L.lib()
    one = Call("persistent")
    f = 0x7E0000200000
    z = _gumbel_args(L).gumbel

    def draw(tree, ids, turns, gz):
        return lib.iago_mcts_gumbel_draw(tree, None, SEED, ids, turns, None if gz is None else C.byref(gz), None), \
            lib.iago_last_error()
    who = b"iago_mcts_gumbel_draw"
    _refused(draw(None, f, f, z), who, b"bad tree")
    _refused(draw(C.byref(one.tree), None, f, z), who, b"null pointer")
    _refused(draw(C.byref(one.tree), f, None, z), who, b"null pointer")
    _refused(draw(C.byref(one.tree), f, f, None), who, b"null gumbel")
    _refused(draw(C.byref(one.tree), f, f, _gumbel_args(L, m=0).gumbel), who, b"m must be")
    _refused(draw(C.byref(one.tree), f, f, _gumbel_args(L, g=None).gumbel), who, b"null table")

    def finish(tree, gz, move, n, q, lg):
        return lib.iago_mcts_gumbel_finish(tree, None, None if gz is None else C.byref(gz), move, n, q, lg, None), \
            lib.iago_last_error()
    who = b"iago_mcts_gumbel_finish"
    _refused(finish(None, z, f, f, f, f), who, b"bad tree")
    for k in range(4):
        ptrs = [f] * 4
        ptrs[k] = None
        _refused(finish(C.byref(one.tree), z, *ptrs), who, b"null pointer")
    _refused(finish(C.byref(one.tree), None, f, f, f, f), who, b"null gumbel")
    _refused(finish(C.byref(one.tree), _gumbel_args(L, c_visit=5000).gumbel, f, f, f, f), who, b"c_visit")


# ---- the engine's arguments
def test_gumbel_arg_and_play_rules():
    from iago_amd import engine, ops
    assert ops.gumbel_arg(None) is None and ops.gumbel_arg((16, 256)) == (16, 256, 50) and ops.gumbel_arg([4, 1, 0]) == (4, 1, 0)
    for bad in ((1, 256), (65, 256), (16, 0), (16, 4097), (16, 256, -1), (16, 256, 4097), (16,), (16, 256, 50, 1), 16,
                (16.0, 256), (True, 256), "ab"):
        with pytest.raises(ValueError, match="gumbel"):
            ops.gumbel_arg(bad)
    r = engine._play_rules(16, gumbel=(16, 256))
    assert r.gumbel == (16, 256, 50) and r[:6] == engine.NO_RULES[:6]
    assert engine._play_rules(16, solve_empties=6, playout_cap=(8, 64), gumbel=(4, 256)).gumbel == (4, 256, 50)
    for kw in (dict(root_noise=(77, 64)), dict(explore_turns=4), dict(root_noise=(77, 0), forced_playouts=512)):
        with pytest.raises(ValueError, match="gumbel is not available together"):
            engine._play_rules(16, gumbel=(16, 256), **kw)
    with pytest.raises(ValueError, match="m must be"):
        engine._play_rules(16, gumbel=(70, 256))
    with pytest.raises(ValueError, match="n_sims"):
        engine._play_rules(40000, gumbel=(16, 256))
    # off is today's record
    assert engine.NO_RULES.gumbel is None and engine.PlayRules(None, 0, None) == engine.NO_RULES
    assert engine._play_rules(32) == engine.NO_RULES


def test_the_engine_refuses_the_wrong_rules_without_a_device():
    from iago_amd import engine
    def check(m, gumbel, **kw):   # (the rule of search()'s arguments, on engine m)
        rule = engine.root_rule(16, gumbel=gumbel, engine=m, **kw)
        return rule and rule.gumbel
    ok = dict(backup="negamax", selection="alphazero", persistent=True, wave_entry=False, rollout_hook=None, use_graph=False,
              async_steps=False, lookahead=0)
    assert check(types.SimpleNamespace(**ok), (16, 256)) == (16, 256, 50)
    assert check(types.SimpleNamespace(), None) is None                              # off: nothing is looked at
    for kw, what in ((dict(backup="reference"), "negamax"), (dict(selection="reference"), "alphazero"),
                     (dict(persistent=False), "persistent search only"), (dict(wave_entry=True), "persistent search only"),
                     (dict(use_graph=True), "persistent search only"), (dict(rollout_hook=print), "persistent search only")):
        with pytest.raises(ValueError, match=what):
            check(types.SimpleNamespace(**{**ok, **kw}), (16, 256))
    with pytest.raises(ValueError, match="root_noise or forced_playouts"):
        check(types.SimpleNamespace(**ok), (16, 256), root_noise=(77, 64))
    with pytest.raises(ValueError, match="m must be"):
        check(types.SimpleNamespace(**ok), (1, 256))
    with pytest.raises(ValueError, match="gumbel is not available"):
        engine.ArenaEngine.play(None, 24, gumbel=(16, 256))
