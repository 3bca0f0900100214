"""The three rollout kernels behind iago_rollout -- 16 lanes per board (throughput_hint 0, both its instances), one
lane per board (1), 8 lanes per board (2) -- against the exact, order-free reference of tests/rollout_exact_ref.py:
power-of-two tables, so every draw is decided in integers with NO tolerance, on probes that read every table
entry a legal cell can read (guarded without a GPU in tests/test_rollout_exact_ref_cpu.py); and with real weights
at the edges of the uniform's range and next to the CDF's boundaries, where the fix-up branches run."""
import numpy as np
import pytest
import torch

from tests import rollout_exact_ref as R

pytestmark = pytest.mark.gpu
HINTS = (0, 1, 2)


@pytest.fixture(scope="module")
def ops():
    from iago_amd import ops as o
    assert torch.cuda.is_available(), "the -m gpu tests need a HIP device"
    return o


class Got(object):
    pass


def run(ops, own, opp, weights, trace=True, uniforms=None, **kw):
    """uniforms: (MAXT, n) float32, or a scalar for every turn of every board."""
    if uniforms is not None:
        if np.ndim(uniforms) == 0:
            uniforms = np.full((R.MAXT, len(own)), uniforms, np.float32)
        assert uniforms.dtype == np.float32
        uniforms = torch.from_numpy(uniforms).cuda()
    res = ops.rollout(ops.bits_to_tensor(own), ops.bits_to_tensor(opp), weights, want_final=True, want_turns=True,
                      want_trace=trace, uniforms=uniforms, **kw)
    torch.cuda.synchronize()
    g = Got()
    g.z, g.n_turns = res.z.cpu().numpy(), res.n_turns.cpu().numpy()
    g.final_own, g.final_opp = ops.tensor_to_bits(res.final_own), ops.tensor_to_bits(res.final_opp)
    g.trace = res.trace.cpu().numpy() if trace else None
    assert (res.trace is not None) == trace
    return g


def first_uniforms(u):
    us = np.zeros((R.MAXT, len(u)), np.float32)
    us[0] = u
    return us


def assert_games_equal(got, want, sel=None, upto=None):
    """Every field of the games `sel` (default: all); upto (n,): the traces only on turns before upto[b], nothing
    else for a board with upto[b] < MAXT (a dropped one)."""
    n = len(want.z)
    sel = np.ones(n, bool) if sel is None else sel
    whole = sel if upto is None else sel & (upto >= R.MAXT)
    if got.trace is not None:
        turns = np.arange(R.MAXT)[:, None]
        cmp_ = whole[None, :] | (False if upto is None else (sel[None, :] & (turns < upto[None, :])))
        bad = np.argwhere((got.trace != want.trace) & cmp_)
        assert len(bad) == 0, ("first mismatches (turn, board)", bad[:5].tolist(), len(bad))
    assert np.array_equal(got.n_turns[whole], want.n_turns[whole])
    assert np.array_equal(got.final_own[whole], want.final_own[whole])
    assert np.array_equal(got.final_opp[whole], want.final_opp[whole])
    assert np.array_equal(got.z[whole], want.z[whole])


# ---- 1. one turn, exact, every kernel -------------------------------------------------------------------

@pytest.mark.parametrize("name", [s[0] for s in R.weight_sets()])
def test_one_turn_exact(ops, name):
    """Planted uniform at turn 0 (random grid points, on a boundary, one step below one), 0 afterwards: trace[0] is
    the integer rule's cell on EVERY kept probe; the rest of the game is the first-legal one (trace with its 0xFE
    past the end, turn count, final boards, z)."""
    _, kw, kb = R.set_by_name(name)
    case = R.one_turn_case(name)
    weights = R.snapped_weights(ops, kw, kb)
    sizes = [len(case.own)] + ([1, 17] if name in ("rich0", "tap000", "bias") else [])
    for n in sizes:
        for hint in HINTS:
            got = run(ops, case.own[:n], case.opp[:n], weights, uniforms=first_uniforms(case.u[:n]), throughput_hint=hint)
            wrong = np.flatnonzero(got.trace[0] != case.cell[:n].astype(np.uint8))
            assert len(wrong) == 0, (name, hint, n, len(wrong), wrong[:5].tolist(), got.trace[0][wrong[:5]].tolist(),
                                     case.cell[wrong[:5]].tolist(), case.group[wrong[:5]].tolist())
            if n == len(case.own):
                assert_games_equal(got, case.game)
            else:
                assert np.array_equal(got.trace, case.game.trace[:, :n]) and np.array_equal(got.z, case.game.z[:n])


# ---- 2. whole games under Philox, exact ----------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(R.PHILOX_KEYS))
def test_whole_games_philox_exact(ops, name):
    """1,027 boards (a third the start position) on their own Philox streams, no planted uniform: the games are the
    reference's, which draws orc.uniform(seed, id_base + b, t, stream) itself -- the production instance
    (rollout_row_kernel<false>: no trace) by z, final boards and turn counts, the others by their full traces too.
    A kept game of more than 64 turns crosses into the second Philox draw."""
    _, kw, kb = R.set_by_name(name)
    own, opp, want = R.philox_case(name)
    seed, id_base, stream = R.PHILOX_KEYS[name]
    assert (~want.kept).sum() <= 0.05 * len(own) and (want.n_turns[want.kept] > 64).any()
    weights = R.snapped_weights(ops, kw, kb)
    keys = dict(seed=seed, id_base=id_base, stream_id=stream)
    assert_games_equal(run(ops, own, opp, weights, trace=False, throughput_hint=0, **keys), want, want.kept)
    for hint in HINTS:
        assert_games_equal(run(ops, own, opp, weights, throughput_hint=hint, **keys), want, want.kept)


# ---- 3. the extremes of the uniform, real weights ----------------------------------------------------

@pytest.mark.parametrize("which", ["shipped", "random"])
def test_extreme_uniforms(ops, which):
    """uniforms = 0 everywhere: every move is the first legal cell, on every board.  uniforms = 1 - 2^-24 everywhere:
    every move is the float64 oracle's draw (the last legal cell unless it holds next to nothing); a board is
    compared up to the first turn where a boundary of the float64 CDF lies within 1e-5 of u (at most 5 % of the
    boards have one).  The second is what drives the fix-up branches of the 16- and 8-lane kernels: float32
    rounding leaves the count at 64 there (counted in test_rollout_exact_ref_cpu.py)."""
    w, b, _ = R.real_weights(which)
    weights = ops.RolloutWeights(w, b)
    assert weights.log_form == 0
    own, opp = R.extreme_boards()
    first = R.first_legal_game(own, opp)
    last = R.extreme_case(which)[0]
    assert (~last.kept).sum() <= 0.05 * len(own)
    for hint in HINTS:
        assert_games_equal(run(ops, own, opp, weights, uniforms=np.float32(0), throughput_hint=hint), first)
        got = run(ops, own, opp, weights, uniforms=R.U_MAX, throughput_hint=hint)
        assert_games_equal(got, last, upto=last.first_drop)
        # every traced move is legal, dropped boards included: the recorded games replay under the rules
        again = R.play(own, opp, lambda t, mover, waiter, playing: (got.trace[t].astype(np.int64), np.ones(len(own), bool)))
        assert_games_equal(got, again)


def test_extreme_uniforms_log_form(ops):
    """The log form (the 8-lane kernel's; its exp2 is not exact and its far-off cells underflow to 0, so next to
    every turn has a boundary within 1e-5 of u = 0 or u = 1 - 2^-24 -- 544 and 562 of these 600 boards meet one, and
    dropping them would leave nothing): every move is followed instead, and must be the float64 oracle's draw, or,
    at such a turn, a legal cell whose CDF interval widened by 1e-5 holds u."""
    w, b, log_form = R.real_weights("log")
    weights = ops.RolloutWeights(w, b)
    assert log_form and weights.log_form == 1
    own, opp = R.extreme_boards()
    for u in (np.float32(0), R.U_MAX):
        got = run(ops, own, opp, weights, uniforms=u)
        again, moves, tolerated = R.replay_constant_u(own, opp, got.trace, w, b, u, log_form=True)
        assert_games_equal(got, again)
        print("log form, u = %g: %d moves, %d of them at a turn with a boundary within 1e-5 of u" % (u, moves, tolerated))
        # the games are the oracle's own up to a tolerated turn and of the same kind after it: the moves decided exactly
        # (no boundary within 1e-5 of u: the oracle's draw or a failure) are at least 0.8 of those of the oracle's own games
        want_moves, want_exact = R.log_form_case(u)
        assert moves >= 0.8 * want_moves and moves - tolerated >= 0.8 * want_exact, (moves, tolerated, want_moves, want_exact)


# ---- 4. next to a boundary, real weights --------------------------------------------------------------

@pytest.mark.parametrize("hint", HINTS)
def test_next_to_a_boundary(ops, hint):
    """2,051 probes, the shipped weights: uniforms[0] = a boundary of the float64 CDF rounded to the 2^-24 grid, one
    step below, one step above; 0 afterwards.  trace[0] is one of the two legal cells the boundary separates (both
    hold more than 1e-4: nothing else is within float32's reach; for the few probes without such a boundary, a
    legal cell whose CDF interval widened by 1e-5 holds u), and the game goes on as the first-legal one."""
    w, b, _ = R.real_weights("shipped")
    weights = ops.RolloutWeights(w, b)
    c = R.boundary_case()
    n = len(c.own)
    assert c.sure.sum() >= 0.9 * n
    for step in (0, -1, 1):
        u = ((c.g + step) * R.GRID).astype(np.float32)
        got = run(ops, c.own, c.opp, weights, uniforms=first_uniforms(u), throughput_hint=hint)
        a = got.trace[0].astype(np.int64)
        ok = (a == c.lo) | (a == c.hi)
        for i in np.flatnonzero(~c.sure):
            lo = c.cdf[i][a[i] - 1] if a[i] > 0 else 0.0
            ok[i] = a[i] in c.acts[i] and lo - R.TOL <= float(u[i]) < c.cdf[i][a[i]] + R.TOL
        assert ok.all(), (step, np.flatnonzero(~ok)[:5].tolist())
        assert_games_equal(got, R.first_legal_game(c.own, c.opp, first=a))
