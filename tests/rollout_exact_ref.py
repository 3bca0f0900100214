"""Exact, order-free reference of the rollout policy's draw (plain numpy, vectorised over boards; nothing taken
from iago_amd, and nothing known of the table blob's layout outside snapped_weights).

The idea (split_exact_ref.py's, for the three rollout kernels): all three state one sampling rule -- the softmax
numerators of the legal cells are summed in cell order, thr = u * total is rounded ONCE to float32 before any
comparison, and the cell is the number of running sums <= thr.  With weights w = k ln 2 for small integers k every
numerator is a power of two; while the total stays below 2^24 (in units of the smallest numerator) every product
and every sum any kernel forms, in whatever order, is exact in float32.  The draw is then decided by integers:

    K(c)  = kb[c] + sum over planes and taps of kw[plane][ky][kx] * plane[c + (ky - 1, kx - 1)]   (0 off the board)
    w_i   = 2^(K(c_i) - K_min) over the legal cells c_1 < .. < c_m,  S_i = w_1 + .. + w_i,  T = S_m
    thr   = float32(float64(u) * T)          (24 bits x 24 bits: the double product is exact, ONE rounding)
    cell  = c_(1 + #{i : S_i <= thr})

The rule does not change under the power-of-two shifts by which the kernels' tables differ (every factor of the
row tables is shifted by its own maximum, every plane of the per-cell tables by its own).  A turn is ORDER-FREE iff
T < 2^24 and K_max - K_min <= 100 over its legal cells; elsewhere a float32 sum may round and the reference
refuses (NotOrderFree).

Geometry (stated here once; this is the board, not any kernel's indexing).  Bit a = 8 row + column of a uint64;
`own` is the side to move (plane 1 of make_state_var), `opp` its opponent (plane 0).
  * row byte: byte r of a board = row r, bit x of it = column x.  The two HALVES of a row are columns 0-3 and 4-7.
  * 9-bit neighbourhood of cell (r, x): bit 3 ky + kx = cell (r + ky - 1, x + kx - 1), zero off the board.
  * 5-bit window of a quad: a QUAD is four cells of one row half (row r, columns 4 h .. 4 h + 3).  Its window in
    kernel row ky is row r + ky - 1 (zero off the board), columns 0-4 for half 0 (window bit j = column j) and
    columns 3-7 for half 1 (window bit j = column 3 + j): the five columns the quad's four 3-wide taps touch.
    The 16-lane kernel holds rows 0-3 (quads 0-7) as they are and rows 4-7 rotated by 180 degrees: ORIENTATION 1
    is the same quad seen on the rotated board -- row 7 - r, the other half, the window's columns mirrored, kernel
    row 2 - ky.  The coverage counts below index an entry by (orientation, ky as that orientation sees it, plane,
    half as it sees it, window as it sees it).
"""
import numpy as np

from oracle import oracle as orc

U64 = np.uint64
F32, F64 = np.float32, np.float64
LN2 = np.log(2.0)
MAXT = 128
PASS, UNWRITTEN = 0xFF, 0xFE
START_OWN, START_OPP = 0x0000000810000000, 0x0000001008000000
GRID = 2.0 ** -24
U_MAX = F32(1.0 - GRID)          # the largest uniform a draw can be
FULL = U64(0xFFFFFFFFFFFFFFFF)
NOT_A = U64(0xFEFEFEFEFEFEFEFE)  # every column but 0
NOT_H = U64(0x7F7F7F7F7F7F7F7F)  # every column but 7
# (shift, towards higher bits, mask of the cells a step may arrive at)
DIRS = [(1, True, NOT_A), (7, True, NOT_H), (8, True, FULL), (9, True, NOT_A),
        (1, False, NOT_H), (7, False, NOT_A), (8, False, FULL), (9, False, NOT_H)]
MUTATIONS = ("planes", "ky", "kx", "rot_upper", "halves", "bias_mirror")


class NotOrderFree(Exception):
    """A turn whose float32 sums could round: the exact reference does not decide it."""


# ---- rules of the game, on bitboards ----------------------------------------------------------------------

def _step(x, d):
    s, up, mask = d
    return ((x << U64(s)) if up else (x >> U64(s))) & mask


def legal_moves(own, opp):
    """Legal cells of the side to move, as a uint64 per board."""
    own, opp = np.asarray(own, U64), np.asarray(opp, U64)
    empty = ~(own | opp)
    out = np.zeros_like(own)
    for d in DIRS:
        t = _step(own, d) & opp
        for _ in range(5):
            t |= _step(t, d) & opp
        out |= _step(t, d) & empty
    return out


def flips(own, opp, cell):
    """The opponent stones a move at `cell` turns over (0 for an illegal cell or cell < 0)."""
    own, opp = np.asarray(own, U64), np.asarray(opp, U64)
    cell = np.asarray(cell, np.int64)
    bit = np.where(cell >= 0, U64(1) << np.maximum(cell, 0).astype(U64), U64(0))
    out = np.zeros_like(own)
    for d in DIRS:
        run = np.zeros_like(own)
        cur = _step(bit, d) & opp
        for _ in range(6):
            run |= cur
            cur = _step(cur, d) & opp
        closed = (_step(run, d) & own) != 0    # the cell behind a contiguous run is the only own one it can meet
        out |= np.where(closed, run, U64(0))
    return out


def popcount(x):
    return unpack(x).sum(axis=1)


def unpack(x):
    """(n,) uint64 -> (n, 64) int64 of 0/1, column c = bit c."""
    x = np.asarray(x, U64).reshape(-1)
    return ((x[:, None] >> np.arange(64, dtype=U64)[None, :]) & U64(1)).astype(np.int64)


# ---- the exponent of a cell ---------------------------------------------------------------------------------

def exponents(own, opp, kw, kb, mutation=None):
    """K (n, 64) int64 of every cell.  kw (2, 3, 3) and kb (64,) integers; plane 0 = opp, plane 1 = own.
    `mutation` (one of MUTATIONS) is a deliberately WRONG variant, for the guard that the data would notice it."""
    kw = np.asarray(kw, np.int64).reshape(2, 3, 3)
    kb = np.asarray(kb, np.int64).reshape(64)
    assert mutation is None or mutation in MUTATIONS, mutation
    if mutation == "planes":
        kw = kw[::-1]
    elif mutation == "ky":
        kw = kw[:, ::-1, :]
    elif mutation == "kx":
        kw = kw[:, :, ::-1]
    elif mutation == "bias_mirror":
        kb = kb[::-1]

    def conv(k):
        acc = 0
        for pl, board in ((0, opp), (1, own)):
            pad = np.zeros((len(np.atleast_1d(own)), 10, 10), np.int64)
            pad[:, 1:9, 1:9] = unpack(board).reshape(-1, 8, 8)
            for ky in range(3):
                for kx in range(3):
                    acc = acc + int(k[pl, ky, kx]) * pad[:, ky:ky + 8, kx:kx + 8]
        return acc

    c = conv(kw)
    if mutation == "rot_upper":      # rows 4-7 (cells 32..63) with the kernel NOT rotated back
        c = np.concatenate([c[:, :4], conv(kw[:, ::-1, ::-1])[:, 4:]], axis=1)
    if mutation == "halves":
        c = c[:, :, [4, 5, 6, 7, 0, 1, 2, 3]]
    return c.reshape(-1, 64) + kb[None, :]


def float_weights(kw, kb):
    """The float32 weights handed to the library: w = float32(kw ln 2) (18,), b = float32(kb ln 2) (64,)."""
    return ((np.asarray(kw, F64).reshape(18) * LN2).astype(F32), (np.asarray(kb, F64).reshape(64) * LN2).astype(F32))


# ---- the draw -----------------------------------------------------------------------------------------------

_CLIP = 40   # 64 weights of 2^40 fit an int64; a spread beyond it is far past the 2^24 guard anyway


def running_sums(legal, K):
    """(legal mask (n, 64) bool, S (n, 64) int64 running sums in cell order with 0 weight on illegal cells,
    T (n,), order_free (n,) bool).  A board without a legal cell has T = 0 and counts as order-free."""
    lm = unpack(legal).astype(bool)
    any_legal = lm.any(axis=1)
    big = np.int64(1) << 40
    kmin = np.where(lm, K, big).min(axis=1)
    kmax = np.where(lm, K, -big).max(axis=1)
    d = np.clip(K - kmin[:, None], 0, _CLIP)
    w = np.where(lm, np.int64(1) << d, 0)
    S = np.cumsum(w, axis=1)
    T = S[:, -1]
    free = ~any_legal | ((T < (1 << 24)) & (kmax - kmin <= 100))
    return lm, S, T, free


def order_free(own, opp, kw, kb):
    """Which boards' next turn the reference decides."""
    return running_sums(legal_moves(own, opp), exponents(own, opp, kw, kb))[3]


def draw(own, opp, kw, kb, u, mutation=None, strict=True):
    """The cell every board's side to move draws with its uniform u (float32, a multiple of 2^-24 below 1);
    -1 where it has no legal move.  strict: raise NotOrderFree if any turn is not order-free (else such a
    board gets the rule's answer computed in integers all the same, for a caller that has dropped it)."""
    legal = legal_moves(own, opp)
    lm, S, T, free = running_sums(legal, exponents(own, opp, kw, kb, mutation))
    if strict and not free.all():
        raise NotOrderFree("%d of %d turns are not order-free" % (int((~free).sum()), len(free)))
    return cell_of(lm, S, T, u)


def cell_of(lm, S, T, u):
    u = np.asarray(u, F32)
    assert np.all((u >= 0) & (u < 1)) and np.all(u.astype(F64) * 2.0 ** 24 % 1.0 == 0), "uniforms lie on the 2^-24 grid"
    thr = (u.astype(F64) * T.astype(F64)).astype(F32)
    cnt = (lm & (S.astype(F64) <= thr.astype(F64)[:, None])).sum(axis=1)
    m = lm.sum(axis=1)
    cnt = np.minimum(cnt, np.maximum(m - 1, 0))           # (never binds on an order-free turn: thr < T there)
    rank = np.cumsum(lm, axis=1) - 1
    cell = np.argmax(lm & (rank == cnt[:, None]), axis=1)
    return np.where(m > 0, cell, -1)


def first_legal(own, opp):
    legal = legal_moves(own, opp)
    lm = unpack(legal).astype(bool)
    return np.where(lm.any(axis=1), np.argmax(lm, axis=1), -1)


# ---- whole games ----------------------------------------------------------------------------------------------

class Games(object):
    """trace (MAXT, n) uint8 (0xFF pass, 0xFE past the end), n_turns, z, final_own / final_opp in the kernels'
    convention (own = the side that was to move at the start), kept (n,) bool: no turn of the game was refused,
    first_drop (n,) the turn a dropped game was dropped at (MAXT for a kept one)."""


def play(own, opp, chooser):
    """Simulate's turn structure: `while stone_num < 64` is looked at once per PAIR of turns; a turn without a move is
    a pass, two passes in a row end the game.  chooser(t, mover, other, live) -> (cells (n,), ok (n,) bool) is
    asked once per turn for every board; only boards with a move and still playing use the answer."""
    me, other = np.array(own, U64).reshape(-1).copy(), np.array(opp, U64).reshape(-1).copy()
    n = len(me)
    stones = popcount(me | other)
    done = stones >= 64
    pass_flg = np.zeros(n, bool)
    nt = np.zeros(n, np.int64)
    trace = np.full((MAXT, n), UNWRITTEN, np.uint8)
    kept = np.ones(n, bool)
    first_drop = np.full(n, MAXT, np.int64)
    for t in range(MAXT):
        mover, waiter = (me, other) if t % 2 == 0 else (other, me)
        live = ~done
        has = legal_moves(mover, waiter) != 0
        playing = live & has
        cells, ok = chooser(t, mover, waiter, playing)
        newly = playing & ~ok & kept
        first_drop[newly] = t
        kept &= ~newly
        cells = np.where(playing, cells, -1)
        f = flips(mover, waiter, cells)
        bit = np.where(playing, U64(1) << np.maximum(cells, 0).astype(U64), U64(0))
        assert np.all((f != 0) == playing), "a chosen cell is a legal one"
        mover |= f | bit        # (views of me / other: updated in place)
        waiter &= ~f
        passing = live & ~has
        stones = np.where(playing, stones + 1, np.where(passing & pass_flg, 64, stones))
        pass_flg = np.where(live, passing, pass_flg)
        trace[t, live] = np.where(playing, cells, PASS)[live].astype(np.uint8)
        nt += live
        if t % 2 == 1:
            done = done | (stones >= 64)
            if done.all():
                break
    g = Games()
    d = popcount(me) - popcount(other)
    g.trace, g.n_turns, g.z = trace, nt, np.sign(d).astype(np.int8)
    g.final_own, g.final_opp, g.kept, g.first_drop = me, other, kept, first_drop
    return g


def first_legal_game(own, opp, first=None):
    """The game under uniforms = 0 from turn 1 on (thr = 0: the first legal cell), turn 0 playing `first`."""
    def chooser(t, mover, waiter, playing):
        if t == 0 and first is not None:
            return np.asarray(first, np.int64), np.ones(len(mover), bool)
        return first_legal(mover, waiter), np.ones(len(mover), bool)
    return play(own, opp, chooser)


def exact_game(own, opp, kw, kb, uniform_of):
    """Whole games by the exact rule; uniform_of(t, boards) -> float32 uniforms of turn t for those board indices.
    A game is dropped (kept = False) at its first turn that is not order-free."""
    def chooser(t, mover, waiter, playing):
        n = len(mover)
        cells, ok = np.full(n, -1, np.int64), np.ones(n, bool)
        idx = np.flatnonzero(playing)
        if len(idx):
            lm, S, T, free = running_sums(legal_moves(mover[idx], waiter[idx]), exponents(mover[idx], waiter[idx], kw, kb))
            cells[idx] = cell_of(lm, S, T, uniform_of(t, idx))
            ok[idx] = free
        return cells, ok
    return play(own, opp, chooser)


def philox_uniforms(seed, id_base, stream):
    def uniform_of(t, boards):
        return np.array([orc.uniform(seed, (id_base + int(b)) & 0xFFFFFFFF, t, stream) for b in boards], F32)
    return uniform_of


# ---- the float64 oracle's game, for real (not snapped) weights ----------------------------------------------

TOL = 1e-5


def oracle_probs(own, opp, w, b, log_form=False):
    """For every board with a legal move: (board index, legal cells, float64 probabilities (64,)) by the oracle:
    RolloutPolicy in float32, masked and renormalised in float64.  log_form: weights so extreme that
    softmax-then-mask is 0/0 -- the float64 softmax over the legal cells of the oracle's float32 logits instead (as
    test_rollout_gpu.py's replay)."""
    states = (unpack(own) + 2 * unpack(opp)).astype(F32).reshape(-1, 8, 8)
    lm = unpack(legal_moves(own, opp)).astype(bool)
    for i in np.flatnonzero(lm.any(axis=1)):
        acts = np.flatnonzero(lm[i]).tolist()
        prob, logits = orc.rollout_policy(orc.make_state_var(states[i], 1), w, b)
        if log_form:
            lg = np.full(64, -np.inf)
            lg[acts] = logits[acts].astype(F64)
            p = np.exp(lg - lg.max())
            p /= p.sum()
        else:
            p = orc.masked_probs(prob, acts)
        yield i, acts, p


def near_boundary(p, acts, u):
    """A boundary of the float64 CDF BETWEEN two legal cells lies within TOL of u."""
    cdf = np.cumsum(p)[acts]
    return bool(np.any(np.abs(cdf[:-1] / cdf[-1] - float(u)) < TOL))


def oracle_game(own, opp, w, b, u, log_form=False, record=None, counts=None):
    """Whole games with the same uniform u at every turn, drawn by the float64 oracle (orc.choice_cdf).  A game is
    dropped at its first turn where a boundary of the float64 CDF between two legal cells lies within TOL of u.
    record: a list that receives (own, opp) arrays of the boards that move, turn by turn.  counts: a list
    [#moves, #moves at a turn with such a boundary] that is added to."""
    def chooser(t, mover, waiter, playing):
        n = len(mover)
        cells, ok = np.full(n, -1, np.int64), np.ones(n, bool)
        idx = np.flatnonzero(playing)
        for j, acts, p in oracle_probs(mover[idx], waiter[idx], w, b, log_form):
            cells[idx[j]] = orc.choice_cdf(p, float(u))
            ok[idx[j]] = not near_boundary(p, acts, u)
            if counts is not None:
                counts[0] += 1
                counts[1] += int(not ok[idx[j]])
        if record is not None:
            record.append((mover[idx].copy(), waiter[idx].copy()))
        return cells, ok
    return play(own, opp, chooser)


def replay_constant_u(own, opp, trace, w, b, u, log_form=False):
    """Follow recorded games (trace (MAXT, n)) whose every turn drew with the uniform u: every recorded move must be
    the float64 oracle's draw, or -- where a boundary of its CDF lies within TOL of u -- a legal cell whose CDF
    interval, widened by TOL, holds u (the tolerance of test_rollout_gpu.py's replay).  Returns (Games replayed by
    these rules from the recorded moves, #moves, #moves that needed the tolerance)."""
    counts = [0, 0]

    def chooser(t, mover, waiter, playing):
        n = len(mover)
        cells, ok = np.full(n, -1, np.int64), np.ones(n, bool)
        idx = np.flatnonzero(playing)
        for j, acts, p in oracle_probs(mover[idx], waiter[idx], w, b, log_form):
            i = idx[j]
            a = int(trace[t, i])
            assert a in acts, ("an illegal move", i, t, a, acts)
            counts[0] += 1
            if near_boundary(p, acts, u):
                cdf = np.cumsum(p) / np.sum(p)
                lo = cdf[a - 1] if a > 0 else 0.0
                assert lo - TOL <= float(u) < cdf[a] + TOL, (i, t, a, float(u), lo, cdf[a])
                counts[1] += 1
                ok[i] = False
            else:
                assert a == orc.choice_cdf(p, float(u)), (i, t, a)
            cells[i] = a
        return cells, ok
    return play(own, opp, chooser), counts[0], counts[1]


# ---- weight sets --------------------------------------------------------------------------------------------

def one_tap_sets():
    out = []
    for pl in range(2):
        for ky in range(3):
            for kx in range(3):
                kw = np.zeros((2, 3, 3), np.int64)
                kw[pl, ky, kx] = 2
                out.append(("tap%d%d%d" % (pl, ky, kx), kw, np.zeros(64, np.int64)))
    return out


def bias_set():
    return ("bias", np.zeros((2, 3, 3), np.int64), (7 * np.arange(64)) % 4)


def rich_set(seed):
    """kw in -2..2 with all 18 taps nonzero, kb in 0..3."""
    rs = np.random.RandomState(1000 + seed)
    kw = rs.choice([-2, -1, 1, 2], size=(2, 3, 3)).astype(np.int64)
    return ("rich%d" % seed, kw, rs.randint(0, 4, 64).astype(np.int64))


RICH_SEEDS = (0, 1, 2)


def weight_sets():
    return one_tap_sets() + [bias_set()] + [rich_set(s) for s in RICH_SEEDS]


def snapped_weights(ops, kw, kb, device="cuda"):
    """ops.RolloutWeights of the float weights with every table entry replaced by the power of two it stands for
    (exp of a float32 sum of k ln 2 is that power up to ~1e-5; the draw is exact only with the power itself).  The
    only place that knows the blob's regions: E [0, N_E), bias [N_E, N_E + 64), 4 mode words, CT (2 x 512) after
    them (csrc/rollout_blob.hpp).  An entry more than 1e-3 from a power of two is a wrongly built one (a wrong
    exponent is off by 0.5 or more)."""
    import torch
    from iago_amd import _lib
    w, b = float_weights(kw, kb)
    weights = ops.RolloutWeights(w, b, device=device)
    assert weights.log_form == 0, "the exact data needs the product form"
    blob = weights.table.cpu().numpy().copy()
    n_e, n_ct = 3 * 2 * 2 * 256 * 4, 2 * 512
    mode = _lib.ROLLOUT_MODE_INDEX
    assert mode == n_e + 64 and mode + 4 + n_ct == _lib.IAGO_ROLLOUT_TABLE_FLOATS == len(blob)
    assert blob[mode] == 1.0
    for lo, hi in ((0, n_e + 64), (mode + 4, mode + 4 + n_ct)):
        v = blob[lo:hi].astype(F64)
        assert np.all(v > 0) and np.all(np.isfinite(v))
        snap = 2.0 ** np.round(np.log2(v))
        rel = np.max(np.abs(snap - v) / snap)
        assert rel <= 1e-3, ("a table entry is not near a power of two", lo, rel)
        blob[lo:hi] = snap.astype(F32)
        assert np.all(blob[lo:hi].astype(F64) == snap)
    weights.table = torch.from_numpy(blob).to(weights.table.device)
    return weights


# ---- probes ---------------------------------------------------------------------------------------------------

N_PROBES = 4099    # 2^12 + 3: the smallest power of two plus three whose first probes attain the coverage below; the
                   # coverage is a property of the positions, so EVERY weight set (one-tap and bias sets too) runs on all of them
DENSITIES = (0.2, 0.33, 0.45)


def _random_board(rs, density):
    r = rs.random_sample(64)
    own = sum(1 << c for c in range(64) if r[c] < density)
    opp = sum(1 << c for c in range(64) if density <= r[c] < 2 * density)
    return own, opp


def probes(n, seed=0):
    """n synthetic positions (own, opp disjoint, at least one legal move, at least one empty cell; not necessarily
    reachable by play).  Probe i does not depend on n.  Every second candidate is a random board (per-colour density
    0.2, 0.33, 0.45 in turn); the others get one row planted: byte v of one colour (v runs through 0..255 for both
    colours, and through every row), the other colour random on the rest of that row -- so that every row byte of
    either plane turns up next to legal cells, full rows included."""
    rs = np.random.RandomState(77 + seed)
    own, opp = [], []
    k = 0
    while len(own) < n:
        o, p = _random_board(rs, DENSITIES[k % 3])
        if k % 2 == 1:
            j = k // 2
            v, colour, row = j % 256, (j // 256) % 2, (j // 512 + j) % 8
            rest = int(rs.randint(0, 256)) & ~v & 0xFF
            if rs.random_sample() < 0.5:
                rest = 0
            a, b = (v, rest) if colour else (rest, v)
            clear = ~(0xFF << (8 * row)) & 0xFFFFFFFFFFFFFFFF
            o = (o & clear) | (a << (8 * row))
            p = (p & clear) | (b << (8 * row))
        k += 1
        if (o | p) == 0xFFFFFFFFFFFFFFFF:
            continue
        if int(legal_moves(np.array([o], U64), np.array([p], U64))[0]) == 0:
            continue
        own.append(o)
        opp.append(p)
    return np.array(own, U64), np.array(opp, U64)


def planted_uniforms(own, opp, kw, kb, seed=0):
    """One uniform per (order-free) probe, and its group: 0 = a random multiple of 2^-24; 1 = the first grid point
    at or above a boundary S_i / T (exactly ON it where S_i 2^24 / T is an integer: those are preferred);
    2 = one grid step below a group-1 point (the last grid point below the boundary, or next to one lying on it).
    Returns (u float32, group, on_boundary bool)."""
    rs = np.random.RandomState(5 + seed)
    lm, S, T, free = running_sums(legal_moves(own, opp), exponents(own, opp, kw, kb))
    n = len(T)
    u = rs.randint(0, 1 << 24, n).astype(np.int64)
    group = rs.choice([0, 0, 1, 2], size=n)
    on = np.zeros(n, bool)
    for i in np.flatnonzero(group > 0):
        s = [int(v) for v in S[i][lm[i]][:-1]]          # boundaries between two legal cells
        if not s or not free[i]:
            group[i] = 0
            continue
        t = int(T[i])
        exact = [v for v in s if (v << 24) % t == 0]
        v = exact[rs.randint(len(exact))] if exact else s[rs.randint(len(s))]
        g = -((-(v << 24)) // t)                        # ceil(v 2^24 / T)
        on[i] = (v << 24) % t == 0
        u[i] = g if group[i] == 1 else g - 1
    assert np.all((u >= 0) & (u < (1 << 24)))
    return (u.astype(F64) * GRID).astype(F32), group, on


# ---- coverage: which table entries the probes' legal cells read -------------------------------------------

def _rows(board):
    """(n, 10) row bytes with a zero row before row 0 and after row 7."""
    b = np.asarray(board, U64)
    out = np.zeros((len(b), 10), np.int64)
    for r in range(8):
        out[:, r + 1] = ((b >> U64(8 * r)) & U64(0xFF)).astype(np.int64)
    return out


def _rev8(v):
    out = np.zeros_like(v)
    for i in range(8):
        out |= ((v >> i) & 1) << (7 - i)
    return out


def coverage(own, opp):
    """Counted over the legal cells of the given probes (geometry of the module docstring):
    t4   (2, 3, 2, 2, 32) bool: (orientation, ky, plane, half, window) occurred at a quad holding a legal cell;
    nbh  (2, 512) bool: (plane, 9-bit neighbourhood) occurred at a legal cell;
    rowb (3, 2, 2, 256) bool: (ky, plane, half, byte): the byte is row r + ky - 1 of that plane for a legal cell
         (r, x) of that half."""
    legal = legal_moves(own, opp)
    lrows = _rows(legal)[:, 1:9]
    t4 = np.zeros((2, 3, 2, 2, 32), bool)
    rowb = np.zeros((3, 2, 2, 256), bool)
    nbh = np.zeros((2, 512), bool)
    planes = (_rows(opp), _rows(own))
    # orientation 1: the board rotated by 180 degrees (row r -> 7 - r, column x -> 7 - x)
    rplanes = tuple(_rev8(p)[:, ::-1] for p in planes)
    rlrows = _rev8(lrows)[:, ::-1]
    for orient, (pls, lr) in enumerate(((planes, lrows), (rplanes, rlrows))):
        for r in range(8):
            true_row = r if orient == 0 else 7 - r
            if (true_row < 4) != (orient == 0):
                continue        # rows 0-3 are held as they are, rows 4-7 rotated
            for half in range(2):
                fed = ((lr[:, r] >> (4 * half)) & 0xF) != 0
                for ky in range(3):
                    for pl in range(2):
                        win = (pls[pl][:, r + ky] >> (3 * half)) & 0x1F
                        t4[orient, ky, pl, half, np.unique(win[fed])] = True
    for r in range(8):
        for half in range(2):
            fed = ((lrows[:, r] >> (4 * half)) & 0xF) != 0
            for ky in range(3):
                for pl in range(2):
                    rowb[ky, pl, half, np.unique(planes[pl][fed, r + ky])] = True
    lm = unpack(legal).astype(bool)
    for pl, board in ((0, opp), (1, own)):
        pad = np.zeros((len(board), 10, 10), np.int64)
        pad[:, 1:9, 1:9] = unpack(board).reshape(-1, 8, 8)
        pat = np.zeros((len(board), 8, 8), np.int64)
        for ky in range(3):
            for kx in range(3):
                pat |= pad[:, ky:ky + 8, kx:kx + 8] << (3 * ky + kx)
        nbh[pl, np.unique(pat.reshape(-1, 64)[lm])] = True
    return t4, nbh, rowb


def reachable():
    """What a legal cell CAN read, by the rules alone (a legal cell is empty, and has an opponent stone beside it):
    t4: for ky = 1 a window with all four of the quad's own cells occupied (window bits 0-3 in half 0, 1-4 in
        half 1, as either orientation sees them) holds no empty cell -- 16 of the 768 entries;
    nbh: the centre bit (4) is clear; plane 0 (the opponent) is never empty around a legal cell, plane 1 (the side to
        move) never holds all eight neighbours -- 255 of the 512 patterns per plane;
    rowb: for ky = 1 the byte has a zero bit in the legal cell's half -- every byte but the 16 with that nibble full."""
    t4 = np.ones((2, 3, 2, 2, 32), bool)
    rowb = np.ones((3, 2, 2, 256), bool)
    for half in range(2):
        cells = 0xF << half
        for w in range(32):
            if w & cells == cells:
                t4[:, 1, :, half, w] = False
        for v in range(256):
            if (v >> (4 * half)) & 0xF == 0xF:
                rowb[1, :, half, v] = False
    nbh = np.zeros((2, 512), bool)
    for v in range(512):
        if not v & 16:
            nbh[0, v] = v != 0
            nbh[1, v] = v != 0x1EF
    return t4, nbh, rowb


# ---- the cases both test files use (computed once per process) ----------------------------------------------

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def set_by_name(name):
    return [s for s in weight_sets() if s[0] == name][0]


class OneTurn(object):
    """The one-turn case of a weight set: its order-free probes (own, opp), their planted uniforms u (group, on),
    the cell the exact rule draws, and the game that follows under uniforms = 0; n_dropped of n_probes."""


def one_turn_case(name):
    def make():
        _, kw, kb = set_by_name(name)
        own, opp = _cached(("probes", 0), lambda: probes(N_PROBES))
        free = order_free(own, opp, kw, kb)
        c = OneTurn()
        c.n_probes, c.n_dropped = len(own), int((~free).sum())
        c.own, c.opp = own[free], opp[free]
        c.u, c.group, c.on = planted_uniforms(c.own, c.opp, kw, kb)
        c.cell = draw(c.own, c.opp, kw, kb, c.u)
        c.game = first_legal_game(c.own, c.opp, first=c.cell)
        return c
    return _cached(("one_turn", name), make)


def positions_by_play(n, seed, n_start):
    """n positions reached by uniformly random oracle playouts cut at a random turn, the first n_start of them the
    start position."""
    from tests.gpu_util import random_positions
    own, opp = random_positions(n, seed=seed)
    own[:n_start], opp[:n_start] = START_OWN, START_OPP
    return own, opp


PHILOX_N = 1027
PHILOX_KEYS = {"rich0": (11, 77, 3), "rich1": (12, 4000000000, 5)}   # seed, id_base, stream_id


def philox_case(name):
    """(own, opp, Games by the exact rule) of the whole-game case of a rich set."""
    def make():
        _, kw, kb = set_by_name(name)
        own, opp = positions_by_play(PHILOX_N, seed=10 + int(name[-1]), n_start=PHILOX_N // 3)
        seed, id_base, stream = PHILOX_KEYS[name]
        return own, opp, exact_game(own, opp, kw, kb, philox_uniforms(seed, id_base, stream))
    return _cached(("philox", name), make)


EXTREME_N = 600


def real_weights(which):
    """(w, b, log form) of the real-weight sets: the shipped and the seeded random weights of simulate.json, and a
    set so extreme that the library takes the log form."""
    from tests.conftest import load_json
    if which == "log":
        rs = np.random.RandomState(3)
        return (12.0 * rs.randn(18)).astype(F32), (5.0 * rs.randn(64)).astype(F32), True
    g = load_json("simulate.json")
    w, b = (g["shipped_w"], g["shipped_b"]) if which == "shipped" else (g["w"], g["b"])
    return np.asarray(w, F32), np.asarray(b, F32), False


def extreme_boards():
    return _cached("extreme_boards", lambda: positions_by_play(EXTREME_N, seed=41, n_start=3))


def extreme_case(which):
    """(Games under u = U_MAX by the float64 oracle, the (own, opp) of every turn that moved) for a product-form set."""
    def make():
        w, b, log_form = real_weights(which)
        assert not log_form
        own, opp = extreme_boards()
        rec = []
        games = oracle_game(own, opp, w, b, U_MAX, record=rec)
        return games, np.concatenate([r[0] for r in rec]), np.concatenate([r[1] for r in rec])
    return _cached(("extreme", which), make)


BOUNDARY_N = 2051


class Boundary(object):
    """The boundary case: probes (own, opp), the grid index g of the float64 CDF boundary behind a randomly chosen
    legal cell, the legal cells lo / hi on either side of it, `sure`: both hold more than TOL of probability, so a
    float32 CDF (good to ~1e-6) can only fall on one of the two; acts / cdf per probe for the others."""


def boundary_case():
    def make():
        w, b, _ = real_weights("shipped")
        c = Boundary()
        c.own, c.opp = probes(BOUNDARY_N, seed=1)
        n = BOUNDARY_N
        rs = np.random.RandomState(9)
        c.g, c.lo, c.hi = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
        c.sure, c.acts, c.cdf = np.zeros(n, bool), [None] * n, [None] * n
        for i, acts, p in oracle_probs(c.own, c.opp, w, b):
            cdf = np.cumsum(p) / np.sum(p)
            c.acts[i], c.cdf[i] = acts, cdf
            if len(acts) == 1:
                c.g[i], c.lo[i], c.hi[i], c.sure[i] = rs.randint(1, (1 << 24) - 1), acts[0], acts[0], True
                continue
            good = [j for j in range(len(acts) - 1) if p[acts[j]] > 10 * TOL and p[acts[j + 1]] > 10 * TOL]
            j = good[rs.randint(len(good))] if good else int(rs.randint(len(acts) - 1))
            c.sure[i] = bool(good)
            c.lo[i], c.hi[i] = acts[j], acts[j + 1]
            c.g[i] = min(max(int(round(cdf[acts[j]] * 2.0 ** 24)), 1), (1 << 24) - 2)
        return c
    return _cached("boundary", make)


def log_form_case(u):
    """(#moves, #moves at a turn WITHOUT a boundary within TOL of u) of the float64 oracle's own games on the extreme
    boards under the log-form weights and the uniform u at every turn: how many moves these data decide exactly."""
    def make():
        w, b, log_form = real_weights("log")
        own, opp = extreme_boards()
        counts = [0, 0]
        oracle_game(own, opp, w, b, u, log_form=log_form, counts=counts)
        return counts[0], counts[0] - counts[1]
    return _cached(("log_form", float(u)), make)
