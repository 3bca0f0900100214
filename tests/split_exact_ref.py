"""Exact, order-free reference of the split-f16 kernels (plain numpy; no arithmetic taken from iago_amd).

The idea (the integer trick of test_conv_gpu.py::test_integer_data_is_exact with the low pieces alive): choose
data for which EVERY sum a kernel forms in an order it does not specify is exact in float32 whatever the order
-- assert_order_free is that condition, called on the very data a test sends to the GPU -- and mirror in float32
every rounding a kernel performs at a place it does specify (the epilogue formula, the re-split, the weight
gradient's group sum).  The result is then known bit for bit: a wrong, missing, doubled or mis-scaled term in any
piece, tap, cell or channel is an exact mismatch.

Conventions: pieces are float16 arrays in the nominal layouts -- weights (128, cin, 3, 3), activations
(n, C, 8, 8), cell = 8 row + column -- and the *_blocks helpers write the layouts the kernels read.  A product sum
("term") is computed in float64, which is exact wherever the guard holds (the guard's bound is far inside 53 bits).
"""
import numpy as np

F32, F16 = np.float32, np.float16
S1 = F32(2.0 ** -11)
S2 = F32(2.0 ** -22)
CLAMP = F32(65000.0)


# ---- splitting ----------------------------------------------------------------------------------------------

def split2(a):
    """float32 -> (hi, lo) f16 with hi = f16(a), lo = f16((a - hi) 2^11): conversions round to nearest even
    (subnormal results included), the float32 difference is exact."""
    a = np.asarray(a, F32)
    hi = a.astype(F16)
    lo = ((a - hi.astype(F32)) * F32(2048.0)).astype(F16)
    return hi, lo


def split3(a):
    """float32 -> (hi, mid, lo) f16 with a == hi + mid 2^-11 + lo 2^-22 (every difference is exact)."""
    a = np.asarray(a, F32)
    hi = a.astype(F16)
    r1 = (a - hi.astype(F32)) * F32(2048.0)
    mid = r1.astype(F16)
    lo = ((r1 - mid.astype(F32)) * F32(2048.0)).astype(F16)
    return hi, mid, lo


def merge2(hi, lo):
    """hi + lo 2^-11 in float32 (exact for a canonical split)."""
    return hi.astype(F32) + lo.astype(F32) * S1


def merge3(hi, mid, lo):
    """((lo S2 + mid S1) + hi) in float32, the order of the policy head."""
    return (lo.astype(F32) * S2 + mid.astype(F32) * S1) + hi.astype(F32)


# ---- product sums and the guard -----------------------------------------------------------------------------

def lsb_exponents(a):
    """(e, nz): the exponent of the lowest set bit of every element (2^e is its weight), and which are non-zero."""
    a = np.abs(np.asarray(a, np.float64))
    nz = a != 0
    m, ex = np.frexp(np.where(nz, a, 1.0))
    mi = (m * 2.0 ** 53).astype(np.int64)
    low = (mi & -mi).astype(np.float64)
    return (np.log2(low).astype(np.int64) + ex - 53), nz


_K = 12   # 2^12 > the number of products of any sum here (1152 per convolution output, 37 x 64 per gradient)


class Term(object):
    """One product sum f(a, b), f bilinear (a convolution, a weight-gradient contraction): its exact value, the sum
    of the products' magnitudes, and per output element q = the smallest lsb of any non-zero product in it, where
    the lsb of a product is taken as lsb(a) lsb(b) (its true lsb is that or larger).
    q by a sum that its largest entry dominates: sum of 2^(-K e) over the products of a level of `a` lies in
    [2^(-K m), 2^(K - K m)) for m the smallest e among them."""

    def __init__(self, contract, a, b):
        a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
        self.value = contract(a64, b64) + 0.0      # (+ 0.0: no negative zeros out of BLAS)
        if not _guarded[0]:
            self.absum = self.q = None
            return
        self.absum = contract(np.abs(a64), np.abs(b64))
        ea, nza = lsb_exponents(a64)
        eb, nzb = lsb_exponents(b64)
        marks = np.where(nzb, np.exp2(-_K * eb.astype(np.float64)), 0.0)
        q = np.full(self.value.shape, np.inf)
        for level in np.unique(ea[nza]):
            s = contract(((ea == level) & nza).astype(np.float64), marks)
            with np.errstate(divide="ignore"):
                m = np.ceil(-np.log2(s) / _K - 1e-9)
            q = np.minimum(q, np.where(s > 0, np.exp2(level + m), np.inf))
        self.q = q


class NoTerm(object):
    """An accumulator nothing is added into."""
    value, absum, q = np.zeros(1), np.zeros(1), np.full(1, np.inf)


def _pad(x):
    return np.pad(np.asarray(x, np.float64), ((0, 0), (0, 0), (1, 1), (1, 1)))


def _conv64(w, x):
    """out[n, co, y, x] = sum over ci, ky, kx of w[co, ci, ky, kx] x[n, ci, y + ky - 1, x + kx - 1] (zero padded)."""
    w = np.asarray(w, np.float64)
    xp = _pad(x)
    out = np.zeros((x.shape[0], w.shape[0], 8, 8))
    for ky in range(3):
        for kx in range(3):
            out += np.einsum("oc,ncyx->noyx", w[:, :, ky, kx], xp[:, :, ky:ky + 8, kx:kx + 8], optimize=True)
    return out


def conv_term(w, x):
    """The forward (and, with transposed weights, backward-data) product sum of one pair of pieces."""
    return Term(_conv64, w, x)


def _wgrad64(dy, x):
    """out[co, ci, ky, kx] = sum over boards and cells of dy[b, co, y, x] x[b, ci, y + ky - 1, x + kx - 1]."""
    dy = np.asarray(dy, np.float64)
    xp = _pad(x)
    out = np.zeros((dy.shape[1], x.shape[1], 3, 3))
    for ky in range(3):
        for kx in range(3):
            out[:, :, ky, kx] = np.einsum("noyx,ncyx->oc", dy, xp[:, :, ky:ky + 8, kx:kx + 8], optimize=True)
    return out


def wgrad_term(dy, x):
    return Term(_wgrad64, dy, x)


def plain_sum_term(x, axes):
    """A plain sum of float32 values over `axes` (the bias gradient of split_scaled, the weight gradient's group
    sum): the 'products' are the values themselves."""
    return Term(lambda a, b: (a * b).sum(axis=axes), np.ones(np.shape(x)), x)


GUARD_LIMIT = 2.0 ** 24
_guarded = [True]


class corrupted(object):
    """with corrupted(): the reference evaluates without the guard -- for the mutation check alone, whose corrupted
    references are compared with the true one, never with a kernel."""

    def __enter__(self):
        _guarded[0] = False

    def __exit__(self, *exc):
        _guarded[0] = True


class NotOrderFree(AssertionError):
    pass


def order_free_ratio(acc):
    """max sum|product| / q of one accumulator = a list of the Terms added into it (0: nothing is added)."""
    q = acc[0].q
    for t in acc[1:]:
        q = np.minimum(q, t.q)
    absum = sum(t.absum for t in acc) + np.zeros(np.shape(q))
    live = np.isfinite(q)
    assert np.all(absum[~live] == 0)
    return float(np.max(absum[live] / q[live])) if np.any(live) else 0.0


def assert_order_free(*accumulators):
    """Every accumulator (a list of Terms) holds sum|product| < 2^24 q: every partial sum, in any order, is a
    multiple of q below 2^24 q, hence a float32, hence exact.  A condition on the data, not a measurement.
    Returns the ratios."""
    if not _guarded[0]:
        return None
    ratios = [order_free_ratio(acc) for acc in accumulators]
    for i, r in enumerate(ratios):
        if not r < GUARD_LIMIT:
            raise NotOrderFree("accumulator %d is not order-free: sum|p| / q = %g >= 2^24" % (i, r))
    return ratios


def _exact32(v):
    out = np.asarray(v, np.float64).astype(F32)
    assert not _guarded[0] or np.array_equal(out.astype(np.float64), v), "a guarded sum is not a float32"
    return out


def _acc32(acc):
    return _exact32(sum(t.value for t in acc))


# ---- the kernels ------------------------------------------------------------------------------------------

TWO_TERMS = ("hh", "hl", "lh")
THREE_TERMS = ("hh", "hm", "mh", "hl", "lh", "mm")
_PIECE = {"h": 0, "m": 1, "l": 2}


def terms_of(kinds, w_pieces, x_pieces, make=conv_term, drop=()):
    """{name: Term}: name 'hm' = (first operand's hi) x (second operand's mid).  Two pieces: (hi, lo); three:
    (hi, mid, lo).  drop: names left out (the mutation check)."""
    def piece(ps, ch):
        return ps[_PIECE[ch] if len(ps) == 3 else {"h": 0, "l": 1}[ch]]
    return {k: make(piece(w_pieces, k[0]), piece(x_pieces, k[1])) for k in kinds if k not in drop}


def _pick(terms, names):
    return [terms[k] for k in names if k in terms] or [NoTerm()]


def epilogue2(main, cross, bias, cross_scale=S1):
    """(cross 2^-11 + main) + bias, clamp to [0, 65000], split2 -- float32, in the order the kernels write it (the
    scaling is a power of two: a fused multiply-add gives the same bits).  Returns (hi, lo, overflow)."""
    v = (cross * F32(cross_scale) + main) + np.asarray(bias, F32)[None, :, None, None]
    over = bool(np.any(~(v <= CLAMP)))
    v = np.minimum(np.maximum(v, F32(0.0)), CLAMP)
    return split2(v) + (over,)


def conv2_forward(w, bias, x, drop=(), cross_scale=S1):
    """conv3x3_split / a layer of the trunks: w = (w_hi, w_lo), x = (x_hi, x_lo) -> (y_hi, y_lo, overflow)."""
    t = terms_of(TWO_TERMS, w, x, drop=drop)
    main, cross = _pick(t, ["hh"]), _pick(t, ["hl", "lh"])
    assert_order_free(main, cross)
    n = x[0].shape[0]
    shape = (n, 128, 8, 8)
    return epilogue2(np.broadcast_to(_acc32(main), shape), np.broadcast_to(_acc32(cross), shape), bias, cross_scale)


def epilogue3(m0, m1, m2, bias, s2=S2):
    """((m2 S2 + m1 S1) + m0) + bias, clamp, split3.  Returns (hi, mid, lo, overflow)."""
    v = ((m2 * F32(s2) + m1 * S1) + m0) + np.asarray(bias, F32)[None, :, None, None]
    over = bool(np.any(~(v <= CLAMP)))
    v = np.minimum(np.maximum(v, F32(0.0)), CLAMP)
    return split3(v) + (over,)


def conv3_forward(w, bias, x, drop=(), s2=S2):
    """A layer of the three-piece policy walk: w = (hi, mid, lo), x = (hi, mid, lo)."""
    t = terms_of(THREE_TERMS, w, x, drop=drop)
    a0, a1, a2 = _pick(t, ["hh"]), _pick(t, ["hm", "mh"]), _pick(t, ["hl", "lh", "mm"])
    # (the kernel keeps hi x hi in two accumulators by tap parity and adds them: both halves and their sum are
    # covered by the guard on the whole)
    assert_order_free(a0, a1, a2)
    shape = (x[0].shape[0], 128, 8, 8)
    return epilogue3(*[np.broadcast_to(_acc32(a), shape) for a in (a0, a1, a2)], bias=bias, s2=s2)


def transposed_weights(w):
    """Backward-data's weight: wt[ci][co][ky][kx] = w[co][ci][2 - ky][2 - kx], padded with zero rows to 128."""
    w = np.asarray(w)
    wt = np.zeros((128, w.shape[0], 3, 3), w.dtype)
    for ky in range(3):
        for kx in range(3):
            wt[:w.shape[1], :, ky, kx] = w[:, :, 2 - ky, 2 - kx].T
    return wt


def conv2_backward_data(w, dy, scale_exp, saved, drop=(), cross_scale=S1):
    """conv_layer<MODE_BWD>: w = (w_hi, w_lo) of the block (128, cin, 3, 3); dy = pieces of the gradient times
    2^scale_exp; saved = pieces of the block's input (cin channels).  dx = ((main + cross 2^-11) 2^-e) where
    saved_hi + saved_lo 2^-11 > 0 (float32), else 0; max_bits = the bits of the largest |dx| (0: none).
    Returns (dx float32 (n, cin, 8, 8), max_bits)."""
    ch = saved[0].shape[1]
    t = terms_of(TWO_TERMS, tuple(transposed_weights(p) for p in w), dy, drop=drop)
    main, cross = _pick(t, ["hh"]), _pick(t, ["hl", "lh"])
    assert_order_free(main, cross)
    shape = (dy[0].shape[0], 128, 8, 8)
    main32, cross32 = np.broadcast_to(_acc32(main), shape), np.broadcast_to(_acc32(cross), shape)
    v = (main32 + cross32 * F32(cross_scale)) * F32(2.0 ** -scale_exp)
    on = (saved[0].astype(F32) + saved[1].astype(F32) * S1) > F32(0.0)
    dx = np.where(on, v[:, :ch], F32(0.0)).astype(F32)
    big = F32(np.max(np.abs(dx))) if dx.size else F32(0.0)
    return dx, int(np.array([big], F32).view(np.uint32)[0])


WGRAD_GROUPS = 32


def conv2_wgrad(dy, x, scale_exp, groups=WGRAD_GROUPS, drop=(), cross_scale=S1):
    """wgrad_split_kernel + wgrad_reduce_kernel: group g takes the boards [g per, (g + 1) per), per = ceil(n /
    groups); part_g = main_g + cross_g 2^-11 (float32); dW = 2^-e (sum of the parts in group order, float32).
    The group sum is guarded too.  Returns dW (128, cin, 3, 3) float32."""
    n = dy[0].shape[0]
    per = (n + groups - 1) // groups
    s = np.zeros((128, x[0].shape[1], 3, 3), F32)
    parts = []
    for g in range(groups):
        lo, hi = g * per, min((g + 1) * per, n)
        if lo >= hi:
            continue
        t = terms_of(TWO_TERMS, tuple(p[lo:hi] for p in dy), tuple(p[lo:hi] for p in x), make=wgrad_term, drop=drop)
        main, cross = _pick(t, ["hh"]), _pick(t, ["hl", "lh"])
        assert_order_free(main, cross)
        part = _acc32(main) + _acc32(cross) * F32(cross_scale)
        parts.append(part)
        s = s + part
    if parts:
        assert_order_free([plain_sum_term(np.stack(parts), 0)])
    return np.ldexp(s, -scale_exp).astype(F32)


def split_scaled(x, max_bits, bias_grad=True):
    """split_scaled_kernel + bias_reduce_kernel on float32 (n, C, 8, 8): e = 13 - exponent(max_bits) (0 when
    max_bits is 0), pieces = split2(x 2^e), bias gradient = the sum over boards and cells (guarded).
    Returns (hi, lo, e, db)."""
    x = np.asarray(x, F32)
    e = 0 if max_bits == 0 else 13 - ((int(max_bits) >> 23) - 127)
    v = np.ldexp(x, e).astype(F32)
    assert np.array_equal(np.ldexp(v.astype(np.float64), -e), x.astype(np.float64))
    hi, lo = split2(v)
    if not bias_grad:
        return hi, lo, e, None
    t = plain_sum_term(x, (0, 2, 3))
    assert_order_free([t])
    return hi, lo, e, _exact32(t.value)


def float_bits(v):
    return int(np.array([v], F32).view(np.uint32)[0])


# ---- layouts, written out index by index ----------------------------------------------------------------

def weight_blocks(w):
    """(128, cin, 3, 3) -> [cin/16][3][3][128][16]."""
    w = np.asarray(w)
    cout, cin = w.shape[0], w.shape[1]
    out = np.empty((cin // 16, 3, 3, cout, 16), w.dtype)
    for cb in range(cin // 16):
        for ky in range(3):
            for kx in range(3):
                out[cb, ky, kx] = w[:, 16 * cb:16 * cb + 16, ky, kx]
    return out


def act_blocks(x):
    """(n, C, 8, 8) -> [n][C/16][64][16]."""
    x = np.asarray(x)
    n, c = x.shape[0], x.shape[1]
    out = np.empty((n, c // 16, 64, 16), x.dtype)
    for cb in range(c // 16):
        for i in range(16):
            out[:, cb, :, i] = x[:, 16 * cb + i].reshape(n, 64)
    return out


def acts_of_blocks(a):
    """[n][C/16][64][16] -> (n, C, 8, 8)."""
    a = np.asarray(a)
    n, nb = a.shape[0], a.shape[1]
    out = np.empty((n, nb * 16, 8, 8), a.dtype)
    for cb in range(nb):
        for i in range(16):
            out[:, 16 * cb + i] = a[:, cb, :, i].reshape(n, 8, 8)
    return out


def head_blocks(w9):
    """Block9's (128, 9) piece [channel][tap] -> the MFMA operand [8 chunks][32 rows][16]: row r < 9 = tap r."""
    w9 = np.asarray(w9)
    out = np.zeros((8, 32, 16), w9.dtype)
    for ch in range(8):
        for tap in range(9):
            out[ch, tap] = w9[16 * ch:16 * ch + 16, tap]
    return out


POLICY_ROW_BYTES = 800


def policy_image(hi, mid, lo):
    """One board's LDS image of the policy walk from (128, 8, 8) pieces: uint8 [64][768] -- per cell row 128 f16
    hi, 128 mid, 128 lo, channel c at byte 2 c (the row's last 32 of 800 bytes are padding, not part of this)."""
    out = np.empty((64, 3, 128), F16)
    for k, p in enumerate((hi, mid, lo)):
        out[:, k, :] = np.asarray(p, F16).reshape(128, 64).T
    return out.reshape(64, 384).view(np.uint8)


# ---- generators (fixed seeds) ---------------------------------------------------------------------------

def rich_layer(seed, cin, pieces=2, density=0.02, scale=1.0, bias_bits=12, bias_range=2.0, bias_offset=None):
    """A sparse layer: every weight piece independent small integers in [-2, 2] (times `scale`, a power of two)
    at `density`; the pieces need not be the split of any float.  bias: multiples of 2^-bias_bits in
    (-bias_range, bias_range); with bias_offset (0.5, for a layer whose output another rich layer reads): an integer
    + bias_offset + a multiple of 2^-bias_bits below 1/16 -- on integer-dominated sums no output is then a tiny
    left-over of a cancellation, whose hi piece would have a tiny lsb and spoil the next layer's guard.
    Returns (pieces tuple of f16 (128, cin, 3, 3), bias float32 (128,))."""
    rs = np.random.RandomState(seed)
    ws = []
    for _ in range(pieces):
        w = rs.randint(-2, 3, (128, cin, 3, 3)) * (rs.rand(128, cin, 3, 3) < density)
        assert np.any(w != 0)
        ws.append((w * float(scale)).astype(F16))
    k = int(bias_range * 2 ** bias_bits)
    b = (rs.randint(-k + 1, k, 128) * 2.0 ** -bias_bits).astype(F32)
    if bias_offset is not None:
        small = rs.randint(-2 ** (bias_bits - 4) + 1, 2 ** (bias_bits - 4), 128) * 2.0 ** -bias_bits
        b = (rs.randint(-2, 2, 128) + bias_offset + small).astype(F32)
    return tuple(ws), b


def identity_layer(cin, pieces=2):
    """Centre tap, 1 on the diagonal of hi (channel c + 64 copies channel c of a 64-channel input), every other
    piece and the bias zero: passes a canonically split activation through bit for bit."""
    hi = np.zeros((128, cin, 3, 3), F16)
    for co in range(128):
        hi[co, co % cin, 1, 1] = 1.0
    return (hi,) + tuple(np.zeros_like(hi) for _ in range(pieces - 1)), np.zeros(128, F32)


def only_pieces(layer, keep):
    """The layer with every weight piece not in `keep` (indices) zeroed."""
    ws, b = layer
    return tuple(w if i in keep else np.zeros_like(w) for i, w in enumerate(ws)), b


def integer_acts(seed, n, c):
    """Directly injected integer pieces: hi in 0..3, lo in -3..3."""
    rs = np.random.RandomState(seed)
    hi = rs.randint(0, 4, (n, c, 8, 8)).astype(F16)
    lo = rs.randint(-3, 4, (n, c, 8, 8)).astype(F16)
    return hi, lo


def subnormal_acts(seed, n, c):
    """hi = k 2^-24 with k in 0..63 (f16 subnormals, far below 2^-14), lo = k 2^-24 with |k| <= 3."""
    rs = np.random.RandomState(seed)
    hi = (rs.randint(0, 64, (n, c, 8, 8)) * 2.0 ** -24).astype(F16)
    lo = (rs.randint(-3, 4, (n, c, 8, 8)) * 2.0 ** -24).astype(F16)
    return hi, lo


def large_acts(seed, n, c):
    """Canonical splits of float32 values in [2^14, 65000) with non-zero lo (and some zeros)."""
    rs = np.random.RandomState(seed)
    v = (2.0 ** 14 + rs.randint(0, (65000 - 2 ** 14) * 4, (n, c, 8, 8)) * 0.25).astype(F32)
    v = np.where(rs.rand(n, c, 8, 8) < 0.5, v, F32(0.0))
    return split2(v)


def stem_like_acts(seed, n, c):
    """Canonical splits of {0} and {I + j 2^-12 : I in 1..3, j in 0..3}."""
    rs = np.random.RandomState(seed)
    v = rs.randint(1, 4, (n, c, 8, 8)) + rs.randint(0, 4, (n, c, 8, 8)) * 2.0 ** -12
    v = np.where(rs.rand(n, c, 8, 8) < 0.5, v, 0.0).astype(F32)
    return split2(v)


def gradient_acts(seed, n, c, density=0.5):
    """Injected gradient pieces: hi in -3..3, lo in -3..3, sparse."""
    rs = np.random.RandomState(seed)
    keep = rs.rand(n, c, 8, 8) < density
    hi = (rs.randint(-3, 4, (n, c, 8, 8)) * keep).astype(F16)
    lo = (rs.randint(-3, 4, (n, c, 8, 8)) * keep).astype(F16)
    return hi, lo


def saved_acts(seed, n, c):
    """A saved activation for the ReLU mask, every sign case of (hi, lo) present: hi in {0, 0, 1, 2}, lo in
    {-1, 0, 1} -- among them hi = 0 with lo > 0 (on), hi = 0 with lo < 0 (off), hi = lo = 0 (off)."""
    rs = np.random.RandomState(seed)
    hi = np.array([0, 0, 1, 2], F16)[rs.randint(0, 4, (n, c, 8, 8))]
    lo = rs.randint(-1, 2, (n, c, 8, 8)).astype(F16)
    return hi, lo


def scaled_input(seed, n, c):
    """float32 values k 2^-10, |k| < 4096 (12 bits: the scaled value has a non-zero lo), sparse."""
    rs = np.random.RandomState(seed)
    k = rs.randint(-4095, 4096, (n, c, 8, 8)) * (rs.rand(n, c, 8, 8) < 0.6)
    return (k * 2.0 ** -10).astype(F32)


# ---- boards and stems -----------------------------------------------------------------------------------

RIM = 0xFF818181818181FF
CORNERS = 0x8100000000000081


def special_boards():
    """(own, opp) uint64: the empty board, a full board, stones only on the rim, only in the corners."""
    rs = np.random.RandomState(12)
    pat = int(rs.randint(0, 2 ** 32)) | (int(rs.randint(0, 2 ** 32)) << 32)
    full = 2 ** 64 - 1
    own = [0, pat, RIM & pat, CORNERS & 0x8000000000000001]
    opp = [0, full & ~pat, RIM & ~pat, CORNERS & ~0x8000000000000001]
    return np.array(own, np.uint64), np.array(opp, np.uint64)


def planes_of(own, opp):
    """(n,) uint64 boards -> float32 planes (n, 2, 8, 8): plane 0 = opp, plane 1 = own, cell a = bit a."""
    out = np.zeros((len(own), 2, 64), F32)
    for b in range(len(own)):
        for a in range(64):
            out[b, 0, a] = (int(opp[b]) >> a) & 1
            out[b, 1, a] = (int(own[b]) >> a) & 1
    return out.reshape(-1, 2, 8, 8)


def stem_from_values(v_empty, v_own, v_opp, extra=None):
    """Block1 weights (64, 2, 3, 3) and biases whose output at a cell is v_empty / v_own / v_opp [channel] by the
    cell's state: bias = v_empty, centre taps = the differences (exact in float32 for the grids used here).
    extra: optional integer weights (64, 2, 3, 3) for the other taps (centre entries ignored)."""
    w1 = np.zeros((64, 2, 3, 3), F32)
    if extra is not None:
        w1[:] = extra
    b1 = np.asarray(v_empty, F32)
    w1[:, 0, 1, 1] = np.asarray(v_opp, F32) - b1
    w1[:, 1, 1, 1] = np.asarray(v_own, F32) - b1
    return w1, b1


def stem_forward(w1, b1, planes):
    """acc = b1; acc = fma(w1[c][j], in[j], acc) for j = (plane, ky, kx) in order; clamp to [0, 65000].  Every step
    must be exact in float32 (asserted), so the fused chain is the plain sum.  Returns float32 (n, 64, 8, 8)."""
    xp = _pad(planes)
    n = planes.shape[0]
    acc = np.broadcast_to(np.asarray(b1, np.float64)[None, :, None, None], (n, 64, 8, 8)).copy()
    for c in range(2):
        for ky in range(3):
            for kx in range(3):
                acc = acc + np.asarray(w1, np.float64)[None, :, c, ky, kx, None, None] * \
                    xp[:, c, None, ky:ky + 8, kx:kx + 8]
                assert np.array_equal(acc.astype(F32).astype(np.float64), acc), "the stem's FMA chain is not exact"
    v = acc.astype(F32)
    return np.minimum(np.maximum(v, F32(0.0)), CLAMP)


def two_piece_stem(seed, neighbours=True):
    """A Value stem: per channel and cell state a value of {0} and {I + j 2^-12 : I in 1..3, j in 0..3} (non-zero
    lo pieces); every eighth channel also counts neighbours with weights in {-1, 0, 1} (the other taps)."""
    rs = np.random.RandomState(seed)

    def vals():
        v = rs.randint(1, 4, 64) + rs.randint(0, 4, 64) * 2.0 ** -12
        return np.where(rs.rand(64) < 0.7, v, 0.0).astype(F32)
    extra = np.zeros((64, 2, 3, 3), F32)
    if neighbours:
        e = rs.randint(-1, 2, (64, 2, 3, 3)) * (rs.rand(64, 2, 3, 3) < 0.25)
        extra[7::8] = e[7::8]
    return stem_from_values(vals(), vals(), vals(), extra)


def three_piece_stem(seed, j_max=4, k_max=4, zero=0.2, base=1.0):
    """A policy stem: values base (1 + j 2^-12 + k 2^-23), j in 1..j_max-1, k in 0..k_max-1 -- the 24 bits float32
    has at 1, so mid and lo are both non-zero -- or 0, per channel and cell state; centre taps only.  base: a power of
    two that moves the whole grid (2^-14: mid and lo pieces in the f16 subnormal range; 2^14: values in [2^14, 65000))."""
    rs = np.random.RandomState(seed)

    def vals():
        v = (1.0 + rs.randint(1, j_max, 64) * 2.0 ** -12 + rs.randint(0, k_max, 64) * 2.0 ** -23) * base
        return np.where(rs.rand(64) < 1.0 - zero, v, 0.0).astype(F32)
    return stem_from_values(vals(), vals(), vals())


# ---- the fused Value forward and the policy walk ------------------------------------------------------------

def value_trunk(w1, b1, layers, planes):
    """Block1 and blocks 2..8 of iago_value_forward_split: the pieces (hi, lo) of the LDS image behind the last
    layer, (n, 128, 8, 8), and whether anything saturated."""
    cur = split2(stem_forward(w1, b1, planes))
    over = False
    for ws, b in layers:
        y = conv2_forward(ws, b, cur)
        cur, over = y[:2], over or y[2]
    return cur, over


def _head_contract(w9, x):
    return np.einsum("ct,ncp->ntp", w9, x.reshape(x.shape[0], x.shape[1], 64), optimize=True)


def value_head_h9(w9, b9, x, drop=(), cross_scale=S1):
    """Block9 of the fused forward: tap maps M[tap][cell'] = sum over c of w9[c][tap] x[c][cell'] in split arithmetic
    (w9 = (hi, lo) pieces (128, 9)), Dm = main + cross 2^-11, then s9[cell] = the in-board Dm[tap][cell + off(tap)]
    added in tap order, h9 = max(s9 + b9, 0) -- float32 in that order.  Returns h9 (n, 64)."""
    t = terms_of(TWO_TERMS, w9, x, make=lambda a, b: Term(_head_contract, a, b), drop=drop)
    main, cross = _pick(t, ["hh"]), _pick(t, ["hl", "lh"])
    assert_order_free(main, cross)
    n = x[0].shape[0]
    dm = np.broadcast_to(_acc32(main), (n, 9, 64)) + np.broadcast_to(_acc32(cross), (n, 9, 64)) * F32(cross_scale)
    s9 = np.zeros((n, 64), F32)
    for tap in range(9):
        for cell in range(64):
            yy, xx = cell // 8 + tap // 3 - 1, cell % 8 + tap % 3 - 1
            if 0 <= yy < 8 and 0 <= xx < 8:
                s9[:, cell] = s9[:, cell] + dm[:, tap, yy * 8 + xx]
    return np.maximum(s9 + F32(b9), F32(0.0))


def rich_head(seed, density=0.15):
    """Block9 pieces (128 channels, 9 taps): small integers in [-2, 2], sparse, both pieces alive; b9."""
    rs = np.random.RandomState(seed)
    ws = tuple((rs.randint(-2, 3, (128, 9)) * (rs.rand(128, 9) < density)).astype(F16) for _ in range(2))
    return ws, F32(rs.randint(-4095, 4096) * 2.0 ** -12)


def selector_head(channel):
    """Block9 pieces that pick `channel` at the centre tap: the head's h9[cell] is then the activation itself."""
    hi = np.zeros((128, 9), F16)
    hi[channel, 4] = 1.0
    return (hi, np.zeros_like(hi)), F32(0.0)


def policy_trunk(w1, b1, layers, planes, upto):
    """Block1 and the first `upto` of blocks 2..8 of the three-piece walk: (hi, mid, lo), saturated."""
    cur = split3(stem_forward(w1, b1, planes))
    over = False
    for ws, b in layers[:upto]:
        y = conv3_forward(ws, b, cur)
        cur, over = y[:3], over or y[3]
    return cur, over


def policy_probs(pieces, w9, b10):
    """The policy head in float64 on the image's exact values: softmax over the cells of sum_c w9[c] x[c] + b10."""
    x = sum(p.astype(np.float64) * s for p, s in zip(pieces, (1.0, 2.0 ** -11, 2.0 ** -22)))
    logit = np.einsum("c,ncp->np", np.asarray(w9, np.float64), x.reshape(x.shape[0], 128, 64))
    logit = logit + np.asarray(b10, np.float64)
    e = np.exp(logit - logit.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)
