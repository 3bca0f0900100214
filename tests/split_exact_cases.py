"""The data sets of test_split_exact_gpu.py with their expected bits, built once per process: the one place the
GPU tests and test_split_exact_ref_cpu.py (guard, mutation check) take builders and seeds from."""
import functools

import numpy as np

from tests import split_exact_ref as R

F32 = np.float32


# ---- a. one layer of conv3x3_split ----------------------------------------------------------------------

LAYER_KINDS = ("integer", "subnormal", "large")
ISOLATIONS = (None, "hl", "lh", "ll")


def layer_inputs(kind, cin, n, isolate=None):
    """(x pieces, (w pieces, bias)).  isolate: 'hl' = only (w_hi, x_lo) alive, 'lh' = only (w_lo, x_hi), 'll' =
    only (w_lo, x_lo) -- the dropped product: the output must be relu(bias)."""
    seed = 1000 + 10 * cin + n
    if kind == "integer":
        x, layer = R.integer_acts(seed, n, cin), R.rich_layer(seed + 1, cin)
    elif kind == "subnormal":
        # outputs in the subnormal range too: the re-split rounds to f16 subnormals
        x, layer = R.subnormal_acts(seed, n, cin), R.rich_layer(seed + 2, cin, bias_bits=24, bias_range=2.0 ** -18)
    elif kind == "large":
        x, layer = R.large_acts(seed, n, cin), R.rich_layer(seed + 3, cin, scale=2.0 ** -6)
    else:
        raise ValueError(kind)
    if isolate is not None:
        zero = np.zeros_like(x[0])
        layer = R.only_pieces(layer, (0,) if isolate[0] == "h" else (1,))
        x = (x[0], zero) if isolate[1] == "h" else (zero, x[1])
    return x, layer


@functools.lru_cache(maxsize=None)
def layer_case(kind, cin, n, isolate=None):
    x, layer = layer_inputs(kind, cin, n, isolate)
    return dict(x=x, layer=layer, want=R.conv2_forward(layer[0], layer[1], x))


# ---- b. conv3x3_split_trunk ------------------------------------------------------------------------------

TRUNK_ORDERS = ("irri", "rrii", "iirr")   # first layer 64 -> 128; i = identity, r = rich
_TRUNK_SEEDS = {"irri": 400, "rrii": 500, "iirr": 600}


def trunk_layers(order, seed, pieces=2, **kw):
    layers, cin = [], 64
    for k, o in enumerate(order):
        layers.append(R.rich_layer(seed + 100 * k, cin, pieces, **kw) if o == "r" else R.identity_layer(cin, pieces))
        cin = 128
    return layers


@functools.lru_cache(maxsize=None)
def trunk_case(order, n):
    """Stem-like activations (64 channels) through two consecutive rich layers among identity layers; `want` is the
    list of every layer's (hi, lo, overflow)."""
    x = R.stem_like_acts(7 + n, n, 64)
    return first_order_free(lambda seed: _trunk_case(x, trunk_layers(order, seed)), _TRUNK_SEEDS[order])


def first_order_free(build, seed, tries=8):
    """build(seed) for the first of seed, seed + 1, .. whose data pass the guard.  (Two rich layers in a row pass it
    at a ratio near 1e6 unless the first one's output holds a tiny odd value -- a near cancellation -- whose hi
    piece has a tiny lsb: about one seed in six.  Which seed is taken depends on the condition alone.)"""
    for s in range(seed, seed + tries):
        try:
            return build(s)
        except R.NotOrderFree:
            continue
    raise AssertionError("no order-free data among %d seeds from %d" % (tries, seed))


def _trunk_case(x, layers):
    want, cur = [], x
    for ws, b in layers:
        y = R.conv2_forward(ws, b, cur)
        want.append(y)
        cur = y[:2]
    return dict(x=x, layers=layers, want=want)


# ---- c. backward-data, weight gradient, split_scaled -------------------------------------------------------

SCALE_EXP = 5


@functools.lru_cache(maxsize=None)
def grad_case(cin, n):
    seed = 2000 + 10 * cin + n
    dy = R.gradient_acts(seed, n, 128)
    x = R.integer_acts(seed + 1, n, cin)
    saved = R.saved_acts(seed + 2, n, cin)
    layer = R.rich_layer(seed + 3, cin)
    dx, max_bits = R.conv2_backward_data(layer[0], dy, SCALE_EXP, saved)
    hi, lo, e, _ = R.split_scaled(dx, max_bits, bias_grad=False)
    return dict(dy=dy, x=x, saved=saved, w=layer[0], dx=dx, max_bits=max_bits, dx_split=(hi, lo, e),
                dw=R.conv2_wgrad(dy, x, SCALE_EXP))


@functools.lru_cache(maxsize=None)
def scaled_case(channels, n):
    x = R.scaled_input(3000 + channels + n, n, channels)
    max_bits = R.float_bits(np.max(np.abs(x)))
    return dict(x=x, max_bits=max_bits, want=R.split_scaled(x, max_bits))


# ---- boards ----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def boards(n_random=5, seed=3):
    """A few reachable positions, then the empty board, a full board, stones only on the rim, only in the
    corners: (own, opp) uint64."""
    from tests.gpu_util import random_positions
    own, opp = random_positions(n_random, seed=seed)
    s_own, s_opp = R.special_boards()
    return np.concatenate([own, s_own]), np.concatenate([opp, s_opp])


# ---- d. the fused Value forward ---------------------------------------------------------------------------

VALUE_RICH = ((0, 6), (3,))      # positions of the rich layers among blocks 2..8, the others identity
_VALUE_SEEDS = {(0, 6): 700, (3,): 800}


def value_layers(rich, seed, pieces=2, **kw):
    """The 7 layers of blocks 2..8: rich at the positions `rich`, identity elsewhere (a rich layer that feeds
    another one gets the bias offset that keeps its outputs away from tiny values: rich_layer)."""
    def one(k):
        cin = 64 if k == 0 else 128
        if k not in rich:
            return R.identity_layer(cin, pieces)
        feeds = any(j > k for j in rich)
        return R.rich_layer(seed + 100 * k, cin, pieces, bias_offset=0.5 if feeds and pieces == 3 else None, **kw)
    return [one(k) for k in range(7)]


@functools.lru_cache(maxsize=None)
def value_trunk_case(rich):
    """The crafted stem, identity layers and rich layers at `rich`, on boards(): `act` = the float32 activations
    behind block 8 (n, 128, 64) that a selector head reveals one (channel, cell) at a time."""
    own, opp = boards()
    planes = R.planes_of(own, opp)
    w1, b1 = R.two_piece_stem(31)

    def build(seed):
        layers = value_layers(rich, seed)
        (hi, lo), over = R.value_trunk(w1, b1, layers, planes)
        assert not over
        return dict(own=own, opp=opp, planes=planes, w1=w1, b1=b1, layers=layers, pieces=(hi, lo),
                    act=R.merge2(hi, lo).reshape(len(own), 128, 64))
    return first_order_free(build, _VALUE_SEEDS[rich])


RIM_CELLS = [c for c in range(64) if c // 8 in (0, 7) or c % 8 in (0, 7)]
PROBE_SAMPLE = [((37 * i + 5) % 128, (RIM_CELLS + [c for c in range(64) if c not in RIM_CELLS])[i % 64])
                for i in range(256)]     # every channel twice, every cell four times


@functools.lru_cache(maxsize=None)
def value_head_case():
    """An identity trunk under a rich block9 (both pieces alive) with a non-zero b9: `h9` (n, 64)."""
    own, opp = boards()
    planes = R.planes_of(own, opp)
    w1, b1 = R.two_piece_stem(32)
    layers = value_layers((), 0)
    (hi, lo), over = R.value_trunk(w1, b1, layers, planes)
    w9, b9 = R.rich_head(33)
    return dict(own=own, opp=opp, planes=planes, w1=w1, b1=b1, layers=layers, pieces=(hi, lo), w9=w9, b9=b9,
                h9=R.value_head_h9(w9, b9, (hi, lo)))


# ---- e. the three-piece policy walk -------------------------------------------------------------------------

# name -> (positions of the rich layers, parts of the launch, stem base, weight scale, alive weight pieces)
POLICY_CASES = {
    "rich0-p2": ((0,), 2, 1.0, 1.0, None),
    "rich0-p7": ((0,), 7, 1.0, 1.0, None),
    "rich12-p2": ((1, 2), 2, 1.0, 1.0, None),
    "rich45-p7": ((4, 5), 7, 1.0, 1.0, None),
    "rich01-p3": ((0, 1), 3, 1.0, 1.0, None),
    "only-w-hi": ((1,), 2, 1.0, 1.0, (0,)),       # hi.hi, hi.mid, hi.lo: each alone in its accumulator
    "only-w-mid": ((1,), 2, 1.0, 1.0, (1,)),      # mid.hi, mid.mid alone in theirs; mid.lo is dropped
    "only-w-lo": ((1,), 2, 1.0, 1.0, (2,)),       # lo.hi alone; lo.mid and lo.lo are dropped
    "only-w-lo-64": ((0,), 2, 1.0, 1.0, (2,)),
    "subnormal": ((1,), 2, 2.0 ** -14, 1.0, None),   # mid and lo pieces of the stem are f16 subnormals
    "large": ((1,), 2, 2.0 ** 14, 2.0 ** -6, None),  # values in [2^14, 65000)
}


def policy_rows(n):
    """Which of boards() a policy case of n rows takes (a reachable position, the rim, the corners first)."""
    return [0, 7, 8, 1, 5, 6][:n]


def observed_layers(parts):
    """The scratch buffer of a launch in `parts` parts holds the image behind this many of blocks 2..8."""
    return 7 * (parts - 1) // parts


@functools.lru_cache(maxsize=None)
def policy_case(name, n):
    rich, parts, base, scale, alive = POLICY_CASES[name]
    own, opp = boards()
    rows = policy_rows(n)
    planes = R.planes_of(own[rows], opp[rows])
    w1, b1 = R.three_piece_stem(41, base=base)
    kw = dict(scale=scale)
    if base < 1.0:
        kw.update(bias_bits=36, bias_range=2.0 ** -24)

    def build(seed):
        layers = value_layers(rich, seed, 3, **kw)
        if alive is not None:
            layers = [R.only_pieces(l, alive) if k in rich else l for k, l in enumerate(layers)]
        pieces, over = R.policy_trunk(w1, b1, layers, planes, observed_layers(parts))
        assert not over
        return dict(own=own, opp=opp, rows=rows, w1=w1, b1=b1, layers=layers, parts=parts, pieces=pieces,
                    stem=R.split3(R.stem_forward(w1, b1, planes)))
    return first_order_free(build, 900 + 10 * len(name))


@functools.lru_cache(maxsize=None)
def policy_head_case(piece):
    """An identity net whose channel c* differs between cells only in k (piece 'lo', gain 2^20) or only in j
    (piece 'mid', gain 2^9): logit - max = 2^-3 times the difference, exactly."""
    own, opp = boards()
    planes = R.planes_of(own, opp)
    w1, b1 = R.three_piece_stem(42, zero=0.0)
    c_star = 21
    steps = np.array([0.0, 1.0, 3.0])                  # empty, own, opp: small enough to stay in the piece
    fixed = 5 * 2.0 ** -12 if piece == "lo" else 3 * 2.0 ** -23
    v = (1.0 + fixed + steps * (2.0 ** -23 if piece == "lo" else 2.0 ** -12)).astype(F32)
    b1[c_star] = v[0]
    w1[c_star, 1, 1, 1], w1[c_star, 0, 1, 1] = v[1] - v[0], v[2] - v[0]
    layers = value_layers((), 0, 3)
    pieces, over = R.policy_trunk(w1, b1, layers, planes, 7)
    w9 = np.zeros(128, F32)
    w9[c_star] = 2.0 ** 20 if piece == "lo" else 2.0 ** 9
    b10 = np.zeros(64, F32)
    assert len(set(np.unique(pieces[{"mid": 1, "lo": 2}[piece]][:, c_star]))) >= 2
    return dict(own=own, opp=opp, w1=w1, b1=b1, layers=layers, w9=w9, b10=b10, pieces=pieces,
                probs=R.policy_probs(pieces, w9, b10))
