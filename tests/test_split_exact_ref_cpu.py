"""tests/split_exact_ref.py and the data sets of test_split_exact_gpu.py, checked without a GPU: every data set
passes the guard, the reference's kept terms add up to an independent float64 convolution minus the documented
dropped terms, its layouts are the ops helpers', the identity layer is the identity, and -- the mutation check --
every data set tells a corrupted reference from the true one."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import split_exact_cases as C
from tests import split_exact_ref as R

F64 = np.float64


def _t(a):
    return torch.from_numpy(np.asarray(a, F64))


def _value(pieces):
    return sum(np.asarray(p, F64) * 2.0 ** (-11 * k) for k, p in enumerate(pieces))


# ---- the guard on every data set -----------------------------------------------------------------------------
# (building a case runs assert_order_free on every accumulator of every layer: a case that exists has passed)

@pytest.mark.parametrize("cin", [64, 128])
@pytest.mark.parametrize("kind", C.LAYER_KINDS)
def test_layer_data_are_order_free(kind, cin):
    for n in (1, 4, 5):
        c = C.layer_case(kind, cin, n)
        t = R.terms_of(R.TWO_TERMS, c["layer"][0], c["x"])
        main, cross = R.assert_order_free([t["hh"]], [t["hl"], t["lh"]])
        assert 0 < main < R.GUARD_LIMIT and 0 < cross < R.GUARD_LIMIT
        hi, lo, over = c["want"]
        assert not over and np.any(lo != 0) and np.any(hi != 0)
        x_hi = np.abs(c["x"][0].astype(np.float32))
        if kind == "subnormal":     # operands AND outputs below the f16 normal range
            assert np.all(x_hi < 2.0 ** -14) and np.any(x_hi > 0)
            assert np.all(np.abs(hi.astype(np.float32)) < 2.0 ** -14)
        if kind == "large":
            assert np.all((x_hi == 0) | ((x_hi >= 2.0 ** 14) & (x_hi < 65000))) and np.any(c["x"][1] != 0)
    for isolate in C.ISOLATIONS[1:]:
        for n in (1, 5):
            C.layer_case("integer", cin, n, isolate)


def test_trunk_value_and_gradient_data_are_order_free():
    for order in C.TRUNK_ORDERS:
        for n in (1, 5):
            c = C.trunk_case(order, n)
            assert not any(w[2] for w in c["want"]) and np.any(c["want"][-1][1] != 0)
    for cin in (64, 128):
        for n in (1, 3, 37):
            c = C.grad_case(cin, n)
            assert np.any(c["dx"] != 0) and np.any(c["dw"] != 0) and c["max_bits"] != 0
            c = C.scaled_case(cin, n)
            assert np.any(c["want"][1] != 0) and np.any(c["want"][3] != 0)
    for rich in C.VALUE_RICH:
        c = C.value_trunk_case(rich)
        assert np.any(c["pieces"][1] != 0)
        stem = R.split2(R.stem_forward(c["w1"], c["b1"], c["planes"]))
        assert np.any(stem[1] != 0)              # the stem's output has non-zero low pieces
    c = C.value_head_case()
    assert np.any(c["h9"] > 0) and all(np.any(p != 0) for p in c["w9"]) and c["b9"] != 0


@pytest.mark.parametrize("name", sorted(C.POLICY_CASES))
def test_policy_data_are_order_free(name):
    def subnormal(p):
        a = np.abs(p.astype(np.float32))
        return np.any((a > 0) & (a < 2.0 ** -14))
    for n in (1, 3):
        c = C.policy_case(name, n)
        assert all(np.any(p != 0) for p in c["stem"])             # hi, mid and lo of the stem all alive
        if name == "subnormal":
            assert subnormal(c["stem"][1]) and subnormal(c["stem"][2]) and subnormal(c["pieces"][2])
        if name == "large":
            v = R.merge3(*c["stem"])
            assert np.all((v == 0) | ((v >= 2.0 ** 14) & (v < 65000)))
    for piece in ("lo", "mid"):
        C.policy_head_case(piece)


def test_the_guard_refuses_what_is_not_order_free():
    x = R.split2(np.full((1, 64, 8, 8), 1.0 + 2.0 ** -12, np.float32))
    w = np.zeros((128, 64, 3, 3), np.float16)
    w[:, :, 1, 1] = 1.0
    w[0, 0, 1, 1] = 2.0 ** -14          # one product 2^-14 among 63 of size 1: still far inside 24 bits
    R.assert_order_free([R.conv_term(w, x[0])])
    big = (x[0].astype(np.float32) * 2.0 ** 11).astype(np.float16)
    with pytest.raises(R.NotOrderFree):
        R.assert_order_free([R.conv_term(w, np.where(np.arange(64)[None, :, None, None] == 0, x[0], big))])
    # q is per output element and per product: an identity layer has one product per output
    ws, b = R.identity_layer(128)
    v = np.random.RandomState(0).rand(2, 128, 8, 8).astype(np.float32) * 100
    assert R.assert_order_free([R.conv_term(ws[0], R.split2(v)[0])])[0] < 2048


# ---- the reference against an independent convolution ------------------------------------------------------

def test_two_piece_terms_are_conv2d_minus_the_dropped_term():
    c = C.layer_case("integer", 128, 5)
    w, x = c["layer"][0], c["x"]
    t = R.terms_of(R.TWO_TERMS, w, x)
    kept = t["hh"].value + (t["hl"].value + t["lh"].value) * 2.0 ** -11
    full = F.conv2d(_t(_value(x)), _t(_value(w)), padding=1).numpy()
    dropped = F.conv2d(_t(x[1]), _t(w[1]), padding=1).numpy() * 2.0 ** -22
    assert np.any(dropped != 0) and np.array_equal(kept, full - dropped)


def test_three_piece_terms_are_conv2d_minus_the_dropped_terms():
    c = C.policy_case("rich12-p2", 3)
    w = c["layers"][1][0]
    x = c["stem"]
    x = tuple(np.concatenate([p, p], 1) for p in x)
    t = R.terms_of(R.THREE_TERMS, w, x)
    kept = t["hh"].value + (t["hm"].value + t["mh"].value) * 2.0 ** -11 + \
        (t["hl"].value + t["lh"].value + t["mm"].value) * 2.0 ** -22
    full = F.conv2d(_t(_value(x)), _t(_value(w)), padding=1).numpy()

    def conv(a, b):
        return F.conv2d(_t(b), _t(a), padding=1).numpy()
    dropped = (conv(w[1], x[2]) + conv(w[2], x[1])) * 2.0 ** -33 + conv(w[2], x[2]) * 2.0 ** -44
    assert np.any(dropped != 0)
    # (float64 holds 2^7 .. 2^-44 only to 2^-45: compare to that)
    assert np.max(np.abs(kept - (full - dropped))) < 2.0 ** -40


def test_gradient_terms_are_autograd_minus_the_dropped_term():
    c = C.grad_case(64, 3)
    w, dy, x = c["w"], c["dy"], c["x"]
    # backward-data: d/dx of sum(conv2d(x, W) * dy) = conv_transpose2d(dy, W)
    t = R.terms_of(R.TWO_TERMS, tuple(R.transposed_weights(p) for p in w), dy)
    kept = (t["hh"].value + (t["hl"].value + t["lh"].value) * 2.0 ** -11)[:, :64]
    full = F.conv_transpose2d(_t(_value(dy)), _t(_value(w)), padding=1).numpy()
    dropped = F.conv_transpose2d(_t(dy[1]), _t(w[1]), padding=1).numpy() * 2.0 ** -22
    assert np.any(dropped != 0) and np.array_equal(kept, full - dropped)
    # weight gradient: d/dW of sum(conv2d(X, W) * dY)
    t = R.terms_of(R.TWO_TERMS, dy, x, make=R.wgrad_term)
    kept = t["hh"].value + (t["hl"].value + t["lh"].value) * 2.0 ** -11

    def dw(dy_, x_):
        wz = torch.zeros(128, 64, 3, 3, dtype=torch.float64, requires_grad=True)
        (F.conv2d(_t(x_), wz, padding=1) * _t(dy_)).sum().backward()
        return wz.grad.numpy()
    assert np.array_equal(kept, dw(_value(dy), _value(x)) - dw(dy[1], x[1]) * 2.0 ** -22)


def test_value_head_terms_are_conv2d():
    c = C.value_head_case()
    w9, x = c["w9"], c["pieces"]
    h9 = R.value_head_h9(w9, c["b9"], x)
    w = _value(w9).reshape(1, 128, 3, 3)
    full = F.conv2d(_t(_value(x)), _t(w), padding=1).numpy()
    dropped = F.conv2d(_t(x[1]), _t(w9[1].astype(F64).reshape(1, 128, 3, 3)), padding=1).numpy() * 2.0 ** -22
    want = np.maximum(full - dropped + float(c["b9"]), 0).reshape(-1, 64)
    assert np.max(np.abs(h9 - want)) < 1e-5 * np.max(want)       # (h9 is rounded to float32 tap by tap)


# ---- layouts ----------------------------------------------------------------------------------------------

def test_layouts_are_the_ops_helpers():
    from iago_amd import ops
    rs = np.random.RandomState(5)
    for cin in (64, 128):
        w = (rs.randn(128, cin, 3, 3) / 30).astype(np.float32)
        hi, lo = ops.split_weights(torch.from_numpy(w))
        rh, rl = R.split2(w)
        assert np.array_equal(hi.numpy(), R.weight_blocks(rh)) and np.array_equal(lo.numpy(), R.weight_blocks(rl))
        p3 = ops.split_weights3(torch.from_numpy(w))
        for got, want in zip(p3, R.split3(w)):
            assert np.array_equal(got.numpy(), R.weight_blocks(want))
        th, tl = ops.split_weights_transposed(torch.from_numpy(w))
        rh, rl = R.split2(R.transposed_weights(w))
        assert np.array_equal(th.numpy(), R.weight_blocks(rh)) and np.array_equal(tl.numpy(), R.weight_blocks(rl))
        x = rs.randn(3, cin, 8, 8).astype(np.float32)
        assert np.array_equal(ops.nchw_to_blocks(torch.from_numpy(x)).numpy(), R.act_blocks(x))
        assert np.array_equal(R.acts_of_blocks(R.act_blocks(x)), x)
    w9 = (rs.randn(1, 128, 3, 3) / 30).astype(np.float32)
    hi, lo = ops.split_head_weights(torch.from_numpy(w9))
    rh, rl = R.split2(w9.reshape(128, 9))
    assert np.array_equal(hi.numpy(), R.head_blocks(rh)) and np.array_equal(lo.numpy(), R.head_blocks(rl))
    assert ops.POLICY_SCRATCH_ROW_BYTES == 64 * R.POLICY_ROW_BYTES and ops.WGRAD_GROUPS == R.WGRAD_GROUPS
    # split3 is exact for float32 values whose pieces stay in the f16 range
    v = (rs.randn(1000) * 10).astype(np.float32)
    assert np.array_equal(_value(R.split3(v)), v.astype(F64))


def test_boards_and_planes():
    own, opp = C.boards()
    assert len(own) == 9 and not np.any(own & opp)
    assert own[5] == 0 and opp[5] == 0                              # empty
    assert (own[6] | opp[6]) == np.uint64(2 ** 64 - 1)              # full
    assert (own[7] | opp[7]) == np.uint64(R.RIM) and (own[8] | opp[8]) == np.uint64(R.CORNERS)
    a = np.arange(64, dtype=np.uint64)
    x = np.stack([((opp[:, None] >> a) & np.uint64(1)), ((own[:, None] >> a) & np.uint64(1))], axis=1)
    assert np.array_equal(R.planes_of(own, opp), x.astype(np.float32).reshape(-1, 2, 8, 8))


# ---- identity layers ----------------------------------------------------------------------------------------

def test_identity_layer_is_the_identity_on_canonical_splits():
    rs = np.random.RandomState(6)
    v = np.where(rs.rand(2, 64, 8, 8) < 0.3, 0, rs.rand(2, 64, 8, 8) * 100).astype(np.float32)
    for pieces, split, fwd in ((2, R.split2, R.conv2_forward), (3, R.split3, R.conv3_forward)):
        x = split(v)
        ws, b = R.identity_layer(64, pieces)
        y = fwd(ws, b, x)
        assert not y[-1]
        for k in range(pieces):
            assert np.array_equal(y[k][:, :64], x[k]) and np.array_equal(y[k][:, 64:], x[k])   # c + 64 copies c
        ws, b = R.identity_layer(128, pieces)
        z = fwd(ws, b, y[:pieces])
        for k in range(pieces):
            assert z[k].tobytes() == y[k].tobytes()


# ---- the mutation check -------------------------------------------------------------------------------------
# For each kernel family and data set: drop one term, scale the lowest accumulator by 2, zero one tap of the lowest
# weight piece at one corner cell, read the lowest activation piece of a neighbouring channel -- the corrupted
# output must differ from the true one in at least one element.

def _differs(a, b):
    return any(np.asarray(p).tobytes() != np.asarray(q).tobytes() for p, q in zip(a, b))


def _spliced_corner(true, mutated):
    """The true outputs with the values of cell (0, 0) taken from `mutated`."""
    out = [np.array(p, copy=True) for p in true]
    for o, m in zip(out, mutated):
        o[..., 0, 0] = m[..., 0, 0]
    return out


CORNER_TAPS = ((1, 1), (1, 2), (2, 1), (2, 2))      # the taps that reach the board from the corner cell (0, 0)


def _mutation_check(run, w, x, kinds, scale_kw, scale, what, taps=CORNER_TAPS):
    """run(w, x, **kw) -> tuple of arrays (n, C, 8, 8); kw: drop=(names), `scale_kw`=the lowest accumulator's scale."""
    with R.corrupted():
        _mutation_check_(run, w, x, kinds, scale_kw, scale, what, taps)


def _mutation_check_(run, w, x, kinds, scale_kw, scale, what, taps):
    true = run(w, x)
    for k in kinds:
        assert _differs(run(w, x, drop=(k,)), true), "%s: dropping %s goes unseen" % (what, k)
    assert _differs(run(w, x, **{scale_kw: np.float32(2.0) * scale}), true), "%s: a doubled lowest accumulator" % what
    for ky, kx in taps:
        low = np.array(w[-1], copy=True)
        low[:, :, ky, kx] = 0
        mutated = _spliced_corner(true, run(tuple(w[:-1]) + (low,), x))
        assert _differs(mutated, true), "%s: tap (%d, %d) of the lowest weight piece at the corner" % (what, ky, kx)
    rolled = tuple(x[:-1]) + (np.roll(x[-1], 1, axis=1),)
    assert _differs(run(w, rolled), true), "%s: the lowest activation piece of the neighbouring channel" % what


def _fwd2(bias):
    return lambda w, x, **kw: R.conv2_forward(w, bias, x, **kw)[:2]


def _fwd3(bias):
    return lambda w, x, **kw: R.conv3_forward(w, bias, x, **kw)[:3]


@pytest.mark.parametrize("cin", [64, 128])
@pytest.mark.parametrize("kind", C.LAYER_KINDS)
def test_mutations_show_in_the_layer_data(kind, cin):
    for n in (1, 4, 5):
        c = C.layer_case(kind, cin, n)
        ws, b = c["layer"]
        _mutation_check(_fwd2(b), ws, c["x"], R.TWO_TERMS, "cross_scale", R.S1, "%s %d %d" % (kind, cin, n))


def _inputs_of_rich_layers(layers, x, forward, pieces):
    """(k, layer, its input) for the rich layers of a chain (the ones with more than one weight piece alive)."""
    cur = x
    for k, (ws, b) in enumerate(layers):
        if np.any(ws[-1] != 0):
            yield k, (ws, b), cur
        cur = forward(ws, b, cur)[:pieces]


def test_mutations_show_in_the_trunk_and_value_data():
    for order in C.TRUNK_ORDERS:
        for n in (1, 5):
            c = C.trunk_case(order, n)
            for k, (ws, b), cur in _inputs_of_rich_layers(c["layers"], c["x"], R.conv2_forward, 2):
                _mutation_check(_fwd2(b), ws, cur, R.TWO_TERMS, "cross_scale", R.S1, "%s %d layer %d" % (order, n, k))
    for rich in C.VALUE_RICH:
        c = C.value_trunk_case(rich)
        stem = R.split2(R.stem_forward(c["w1"], c["b1"], c["planes"]))
        for k, (ws, b), cur in _inputs_of_rich_layers(c["layers"], stem, R.conv2_forward, 2):
            _mutation_check(_fwd2(b), ws, cur, R.TWO_TERMS, "cross_scale", R.S1, "value %s layer %d" % (rich, k))


@pytest.mark.parametrize("name", sorted(C.POLICY_CASES))
def test_mutations_show_in_the_policy_data(name):
    rich, _, _, _, alive = C.POLICY_CASES[name]
    # with one weight piece alive only that piece's kept products exist; it is then the lowest weight piece, and the
    # lowest activation piece is the lowest one it has a kept product with (hi: lo, mid: mid, lo: hi)
    kinds = [k for k in R.THREE_TERMS if alive is None or "hml".index(k[0]) in alive]
    low_w = 2 if alive is None else alive[0]
    low_x = 2 - low_w if alive is not None else 2
    for n in (1, 3):
        c = C.policy_case(name, n)
        assert max(rich) < C.observed_layers(c["parts"])           # the scratch image is behind every rich layer
        with R.corrupted():
            cur = c["stem"]
            for k, (ws, b) in enumerate(c["layers"][:C.observed_layers(c["parts"])]):
                true = R.conv3_forward(ws, b, cur)[:3]
                if k in rich:
                    run = _fwd3(b)
                    for kind in kinds:
                        assert _differs(run(ws, cur, drop=(kind,)), true), (name, n, k, kind)
                    assert _differs(run(ws, cur, s2=np.float32(2.0) * R.S2), true), (name, n, k, "S2")
                    rolled = list(cur)
                    rolled[low_x] = np.roll(cur[low_x], 1, axis=1)
                    assert _differs(run(ws, tuple(rolled)), true), (name, n, k, "channel")
                    for ky, kx in CORNER_TAPS:
                        mw = [np.array(w, copy=True) for w in ws]
                        mw[low_w][:, :, ky, kx] = 0
                        assert _differs(_spliced_corner(true, run(tuple(mw), cur)), true), (name, n, k, "tap", ky, kx)
                cur = true


@pytest.mark.parametrize("cin", [64, 128])
def test_mutations_show_in_the_gradient_data(cin):
    for n in (1, 3, 37):
        c = C.grad_case(cin, n)

        def bwd(w, dy, **kw):
            return (R.conv2_backward_data(w, dy, C.SCALE_EXP, c["saved"], **kw)[0],)
        # (backward-data reads the weights flipped: from the corner the taps 0..1 of the block's weight are in reach)
        _mutation_check(bwd, c["w"], c["dy"], R.TWO_TERMS, "cross_scale", R.S1, "bwd %d %d" % (cin, n),
                        taps=((0, 0), (0, 1), (1, 0), (1, 1)))

        def wgrad(dy, x, **kw):
            return (R.conv2_wgrad(dy, x, C.SCALE_EXP, **kw),)
        with R.corrupted():
            true = wgrad(c["dy"], c["x"])
            for k in R.TWO_TERMS:
                assert _differs(wgrad(c["dy"], c["x"], drop=(k,)), true), k
            assert _differs(wgrad(c["dy"], c["x"], cross_scale=np.float32(2.0) * R.S1), true)
            low = np.array(c["dy"][1], copy=True)
            low[:, :, 0, 0] = 0                          # the lowest piece of the first operand at the corner cell
            assert _differs(wgrad((c["dy"][0], low), c["x"]), true)
            assert _differs(wgrad(c["dy"], (c["x"][0], np.roll(c["x"][1], 1, axis=1))), true)
        # the ReLU mask: testing hi alone would switch off the cells that only lo switches on
        hi_only = np.where(c["saved"][0] > 0, c["dx"], np.float32(0))
        assert not np.array_equal(hi_only, c["dx"])


def test_mutations_show_in_the_value_head_data():
    c = C.value_head_case()
    w9, b9, x = c["w9"], c["b9"], c["pieces"]
    true = (c["h9"],)
    with R.corrupted():
        for k in R.TWO_TERMS:
            assert _differs((R.value_head_h9(w9, b9, x, drop=(k,)),), true), k
        assert _differs((R.value_head_h9(w9, b9, x, cross_scale=np.float32(2.0) * R.S1),), true)
        for tap in (4, 5, 7, 8):                            # the taps that reach the board from cell 0
            low = np.array(w9[1], copy=True)
            low[:, tap] = 0
            mutated = np.array(c["h9"], copy=True)
            mutated[:, 0] = R.value_head_h9((w9[0], low), b9, x)[:, 0]
            assert _differs((mutated,), true), tap
        assert _differs((R.value_head_h9(w9, b9, (x[0], np.roll(x[1], 1, axis=1))),), true)
    # the selector head of the trunk probe reveals exactly the activation
    sel, zero = R.selector_head(17)
    assert np.array_equal(R.value_head_h9(sel, zero, x), R.merge2(*x)[:, 17].reshape(-1, 64))


def test_policy_head_data_tell_the_scales_apart():
    for piece, wrong in (("lo", (1.0, 2.0 ** -11, 2.0 ** -21)), ("mid", (1.0, 2.0 ** -10, 2.0 ** -22))):
        c = C.policy_head_case(piece)
        x = sum(p.astype(F64) * s for p, s in zip(c["pieces"], wrong))
        logit = np.einsum("c,ncp->np", c["w9"].astype(F64), x.reshape(-1, 128, 64))
        e = np.exp(logit - logit.max(axis=1, keepdims=True))
        bad = e / e.sum(axis=1, keepdims=True)
        assert np.max(np.abs(bad - c["probs"]) / c["probs"]) > 0.1       # tens of percent, against a bar of 1e-5
        swapped = R.policy_probs((c["pieces"][0], c["pieces"][2], c["pieces"][1]), c["w9"], c["b10"])
        assert np.max(np.abs(swapped - c["probs"])) > 1e-3
