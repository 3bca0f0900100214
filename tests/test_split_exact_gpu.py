"""Every term of the split-f16 kernels against tests/split_exact_ref.py, bit for bit: data whose sums are exact in
float32 in any order (the guard runs inside every test, on the very data sent to the GPU), low pieces alive."""
import numpy as np
import pytest
import torch

from tests import split_exact_cases as C
from tests import split_exact_ref as R

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _acts(pieces):
    from iago_amd import ops
    hi, lo = pieces
    return ops.SplitActs(_dev(R.act_blocks(hi)), _dev(R.act_blocks(lo)), hi.shape[1])


def _layer(layer):
    ws, b = layer
    return tuple(_dev(R.weight_blocks(w)) for w in ws) + (_dev(b),)


def _same(got, want, what):
    """Bytes of a device tensor against a numpy array of the same dtype and shape."""
    g = got.detach().cpu().numpy()
    assert g.dtype == want.dtype and g.shape == want.shape, (what, g.dtype, g.shape, want.dtype, want.shape)
    if g.tobytes() != np.ascontiguousarray(want).tobytes():
        bad = np.argwhere(g.view(np.uint16 if g.itemsize == 2 else np.uint32)
                          != np.ascontiguousarray(want).view(np.uint16 if g.itemsize == 2 else np.uint32))
        first = tuple(bad[0])
        raise AssertionError("%s: %d of %d words differ, first at %s: got %r, want %r"
                             % (what, len(bad), g.size, first, g[first], want[first]))


def _same_acts(got, want, what):
    _same(got.hi, R.act_blocks(want[0]), what + " hi")
    _same(got.lo, R.act_blocks(want[1]), what + " lo")


# ---- a. conv3x3_split, per layer ------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 4, 5])
@pytest.mark.parametrize("cin", [64, 128])
@pytest.mark.parametrize("kind", C.LAYER_KINDS)
def test_layer_is_exact(kind, cin, n):
    """Injected pieces (integers; hi pieces that are f16 subnormals; values in [2^14, 65000) with non-zero lo),
    sparse weights with both pieces alive: hi, lo and the overflow word (0) bit for bit.
    The subnormal case pins that the f16 MFMAs take subnormal operands as they are: the reference flushes nothing."""
    from iago_amd import ops
    c = C.layer_case(kind, cin, n)          # (the guard ran on these data inside conv2_forward)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = ops.conv3x3_split(_acts(c["x"]), *_layer(c["layer"]), overflow=flag)
    _same_acts(got, c["want"], "%s cin %d n %d" % (kind, cin, n))
    assert int(flag.item()) == int(c["want"][2]) == 0


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("cin", [64, 128])
@pytest.mark.parametrize("isolate", ["hl", "lh", "ll"])
def test_layer_products_one_at_a_time(isolate, cin, n):
    """Only (w_hi, x_lo), only (w_lo, x_hi), only (w_lo, x_lo) alive: the last one is the dropped product and must
    give exactly relu(bias)."""
    from iago_amd import ops
    c = C.layer_case("integer", cin, n, isolate)
    got = ops.conv3x3_split(_acts(c["x"]), *_layer(c["layer"]))
    _same_acts(got, c["want"], "only %s" % isolate)
    if isolate == "ll":
        relu_b = np.broadcast_to(np.maximum(c["layer"][1], 0)[None, :, None, None], (n, 128, 8, 8))
        assert np.array_equal(R.merge2(*c["want"][:2]), relu_b)
    else:
        assert np.any(c["want"][1] != 0)


# ---- b. conv3x3_split_trunk -------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("order", C.TRUNK_ORDERS)
def test_trunk_is_exact_and_equals_the_layers(order, n):
    """Two rich layers in a row behind, between and in front of identity layers, first layer 64 -> 128: the trunk
    launch and the per-layer launches both give the reference's bytes (so, on these data, each other's)."""
    from iago_amd import ops
    c = C.trunk_case(order, n)
    layers = [_layer(l) for l in c["layers"]]
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = ops.conv3x3_split_trunk(_acts(c["x"]), layers, overflow=flag)
    cur = _acts(c["x"])
    for k, l in enumerate(layers):
        cur = ops.conv3x3_split(cur, *l, overflow=flag)
        _same_acts(cur, c["want"][k], "%s layer %d, per layer" % (order, k))
    _same_acts(got, c["want"][-1], "%s trunk" % order)
    assert torch.equal(got.hi, cur.hi) and torch.equal(got.lo, cur.lo)
    assert int(flag.item()) == 0
    for k in range(1, len(layers) + 1):     # every prefix: the layer a defect sits in is named
        part = ops.conv3x3_split_trunk(_acts(c["x"]), layers[:k])
        _same_acts(part, c["want"][k - 1], "%s trunk of %d layers" % (order, k))


# ---- c. backward-data, weight gradient, split_scaled ------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 3, 37])
@pytest.mark.parametrize("cin", [64, 128])
def test_gradient_kernels_are_exact(cin, n):
    """Injected dy, x and saved pieces, scale_exp = 5: dx and max_bits of backward-data (the mask is saved_hi +
    saved_lo 2^-11 > 0: hi = 0 with lo > 0 is ON), the pieces and the published exponent of split_scaled on that
    dx, and dW (32 board groups, ragged at n = 37, empty at n = 1 and 3)."""
    from iago_amd import ops
    c = C.grad_case(cin, n)
    on_by_lo = (c["saved"][0] == 0) & (c["saved"][1] > 0)
    assert np.any(on_by_lo & (c["dx"] != 0)) and np.any((c["saved"][0] == 0) & (c["saved"][1] < 0))
    se = torch.tensor([C.SCALE_EXP], dtype=torch.int32, device="cuda")
    wt = [_dev(R.weight_blocks(R.transposed_weights(p))) for p in c["w"]]
    dy = _acts(c["dy"])
    dx, mb = ops.conv3x3_bwd_data_split(dy, se, wt[0], wt[1], _acts(c["saved"]))
    _same(dx, R.act_blocks(c["dx"]), "dx")
    assert int(mb.item()) == c["max_bits"]
    a, e = ops.split_scaled(dx, mb)
    _same_acts(a, c["dx_split"][:2], "split_scaled(dx)")
    assert int(e.item()) == c["dx_split"][2]
    dw = ops.conv3x3_wgrad_split(dy, _acts(c["x"]), scale_exp=se)
    _same(dw, c["dw"], "dW")


@pytest.mark.parametrize("n", [1, 3, 37])
@pytest.mark.parametrize("channels", [64, 128])
def test_split_scaled_and_bias_gradient_are_exact(channels, n):
    from iago_amd import ops
    c = C.scaled_case(channels, n)
    hi, lo, e, db = c["want"]
    mb = torch.tensor([c["max_bits"]], dtype=torch.int32, device="cuda")
    a, ge, gdb = ops.split_scaled(_dev(R.act_blocks(c["x"])), mb, bias_grad=True)
    _same_acts(a, (hi, lo), "split_scaled")
    assert int(ge.item()) == e and np.any(lo != 0)
    _same(gdb, db, "bias gradient")


# ---- d. the fused Value forward ------------------------------------------------------------------------------

VALUE_FORMS = ("planes", "boards", "gather", "batch2", "batch4", "rows260", "rows515")


class _ValueProbe(object):
    """ops.value_forward_split on a case's stem and layers with selector heads: every tensor is built once, a
    launch only picks its views (no word is rewritten between launches)."""

    def __init__(self, c):
        from iago_amd import ops
        self.ops, self.c = ops, c
        self.n = len(c["own"])
        self.w1, self.b1 = _dev(c["w1"]), _dev(c["b1"])
        self.layers = [_layer(l) for l in c["layers"]]
        heads = np.stack([R.head_blocks(R.selector_head(ch)[0][0]) for ch in range(128)])
        self.sel_hi = _dev(heads)                                   # [channel][8][32][16]
        self.zero_lo = torch.zeros((8, 32, 16), dtype=torch.float16, device="cuda")
        self.b9_zero = torch.zeros(1, dtype=torch.float32, device="cuda")
        w10 = np.zeros((128, 64), np.float32)
        w10[np.arange(64), np.arange(64)] = 1.0                    # fc10 row j < 64 picks cell j
        self.w10 = _dev(w10)
        w11 = np.zeros((64, 1, 128), np.float32)
        w11[np.arange(64), 0, np.arange(64)] = 1.0                 # fc11 one-hot k
        self.w11 = _dev(w11)
        self.flag = torch.zeros(1, dtype=torch.int32, device="cuda")

    def rows(self, form):
        """The board of boards() behind every row of the form's batch."""
        total = {"rows260": 260, "rows515": 515}.get(form, self.n)
        return np.arange(total) % self.n

    def run(self, form, probes, head=None, b9=None):
        """out[i][row] for probe i = (channel, cell) (head given: only the cell counts)."""
        ops, c = self.ops, self.c
        rows = self.rows(form)
        own, opp = ops.bits_to_tensor(c["own"][rows]), ops.bits_to_tensor(c["opp"][rows])
        x = _dev(c["planes"]) if form == "planes" else (own, opp)
        out = torch.full((len(probes), len(rows)), -77.0, dtype=torch.float32, device="cuda")
        kw = {}
        if form == "gather":
            # the rows in reverse order, the last one beyond the device count: its value must stay untouched
            kw = dict(index=torch.arange(len(rows) - 1, -1, -1, device="cuda"),
                      n_dev=torch.tensor([len(rows) - 1], dtype=torch.int32, device="cuda"))
        elif form.startswith("batch"):
            # few workgroups: each walks several passes with the grid's stride
            kw = dict(n_dev=torch.tensor([len(rows)], dtype=torch.int32, device="cuda"),
                      batch=(int(form[5:]), 2 if form == "batch2" else 1))
        for i, (ch, cell) in enumerate(probes):
            hd = head if head is not None else (self.sel_hi[ch], self.zero_lo)
            ops.value_forward_split(x, self.w1, self.b1, self.layers, hd, None, self.b9_zero if b9 is None else b9,
                                    self.w10, self.w11[cell], overflow=self.flag, out=out[i], **kw)
        got = out.cpu().numpy()
        assert int(self.flag.item()) == 0
        return got, rows

    def check(self, form, got, rows, want):
        """want[i][board]; the gather form leaves the row beyond the count (board 0, listed last) alone."""
        want = want[:, rows].copy()
        if form == "gather":
            want[:, 0] = -77.0
        if got.tobytes() != np.ascontiguousarray(want).tobytes():
            bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
            raise AssertionError("%s: %d of %d values differ, first (probe, row) %s: got %r, want %r"
                                 % (form, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


@pytest.fixture(scope="module", params=C.VALUE_RICH, ids=lambda r: "rich" + "".join(map(str, r)))
def value_probe(request):
    return _ValueProbe(C.value_trunk_case(request.param))


@pytest.mark.parametrize("form", VALUE_FORMS)
def test_value_forward_trunk_probe(value_probe, form):
    """The crafted stem, identity layers and one or two rich layers; a selector head (w9 one-hot on the centre tap
    of a channel, b9 = 0, fc10 picks cells, fc11 one-hot) makes the output the activation [channel, cell] itself:
    256 (channel, cell) pairs -- every channel twice, every cell four times -- in every form of the launch: planes,
    boards (one board per workgroup), a gather list with a device count, the device-counted batch form with two and
    four boards per workgroup, and host-known row counts that pick two (260) and four (515) boards per workgroup."""
    act = value_probe.c["act"]
    want = np.stack([act[:, ch, cell] for ch, cell in C.PROBE_SAMPLE])
    got, rows = value_probe.run(form, C.PROBE_SAMPLE)
    value_probe.check(form, got, rows, want)


def test_value_forward_trunk_probe_every_channel_and_cell():
    """The plain form (boards in, one board per workgroup) over all 128 x 64 (channel, cell) pairs."""
    probe = _ValueProbe(C.value_trunk_case(C.VALUE_RICH[0]))
    probes = [(ch, cell) for ch in range(128) for cell in range(64)]
    act = probe.c["act"]
    got, rows = probe.run("boards", probes)
    probe.check("boards", got, rows, np.ascontiguousarray(act.reshape(len(rows), 128 * 64).T))


@pytest.mark.parametrize("form", ["planes", "boards", "batch2", "batch4", "rows515"])
def test_value_forward_head_probe(form):
    """An identity trunk under a rich block9 -- w9_hi and w9_lo both sparse and alive, b9 non-zero -- with fc10 =
    cell selector and fc11 one-hot k over all 64 cells: the 9-row MFMA product and its nine shifted adds on non-zero
    low pieces, against the mirrored head epilogue."""
    c = C.value_head_case()
    probe = _ValueProbe(c)
    head = tuple(_dev(R.head_blocks(p)) for p in c["w9"])
    b9 = torch.tensor([float(c["b9"])], dtype=torch.float32, device="cuda")
    got, rows = probe.run(form, [(0, k) for k in range(64)], head=head, b9=b9)
    probe.check(form, got, rows, np.ascontiguousarray(c["h9"].T))


# ---- e. the three-piece SLPolicy forward -----------------------------------------------------------------------

def _policy_args(c):
    layers = [tuple(_dev(R.weight_blocks(w)) for w in ws) + (_dev(b),) for ws, b in c["layers"]]
    return _dev(c["w1"]), _dev(c["b1"]), layers


@pytest.mark.parametrize("gather", [False, True], ids=["rows", "gather"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name", sorted(C.POLICY_CASES))
def test_policy_walk_image_is_exact(name, n, gather):
    """The LDS image of ops.policy_forward_split3 itself, read from the scratch buffer of a launch in parts (behind
    layers [0, 7 (p - 1) // p) of blocks 2..8): 64 cell rows of 800 B = 128 f16 hi, 128 mid, 128 lo (the last 32 B
    are padding, not compared).  Rich layers at position 0 (64 input channels: two chunk pairs), at 128-channel
    positions with a second rich layer behind; weight pieces alive one at a time (each of the six kept products is
    then alone in its accumulator in one of the runs, and the three dropped ones would show in the others); stem
    pieces that are f16 subnormals; values in [2^14, 65000)."""
    from iago_amd import ops
    c = C.policy_case(name, n)
    w1, b1, layers = _policy_args(c)
    rows = c["rows"]
    kw = {}
    if gather:
        own, opp = ops.bits_to_tensor(c["own"]), ops.bits_to_tensor(c["opp"])
        kw = dict(index=torch.tensor(rows, dtype=torch.int64, device="cuda"),
                  n_dev=torch.tensor([n], dtype=torch.int32, device="cuda"))
    else:
        own, opp = ops.bits_to_tensor(c["own"][rows]), ops.bits_to_tensor(c["opp"][rows])
    scratch = torch.zeros(n * ops.POLICY_SCRATCH_ROW_BYTES, dtype=torch.uint8, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    w9 = torch.ones(128, dtype=torch.float32, device="cuda")
    b10 = torch.zeros(64, dtype=torch.float32, device="cuda")
    ops.policy_forward_split3(own, opp, w1, b1, layers, w9, b10, overflow=flag, parts=c["parts"], scratch=scratch, **kw)
    img = scratch.cpu().numpy().reshape(n, 64, R.POLICY_ROW_BYTES)[:, :, :768]
    assert int(flag.item()) == 0
    for b in range(n):
        want = R.policy_image(*[p[b] for p in c["pieces"]])
        if img[b].tobytes() != want.tobytes():
            g, w = np.ascontiguousarray(img[b]).view(np.float16), want.view(np.float16)
            bad = np.argwhere(g.view(np.uint16) != w.view(np.uint16))
            cell, at = bad[0]
            raise AssertionError("%s row %d: %d of %d words differ, first at cell %d, piece %s, channel %d: got %r, "
                                 "want %r" % (name, b, len(bad), g.size, cell, ("hi", "mid", "lo")[at // 128], at % 128,
                                              g[cell, at], w[cell, at]))


@pytest.mark.parametrize("piece", ["lo", "mid"])
def test_policy_head_reconstructs_the_low_pieces(piece):
    """w9 = 2^20 one-hot(c*) (2^9 for mid), b10 = 0, channel c* differing between cells only in k (in j): logit -
    max is 2^-3 times the difference exactly, so the probabilities follow from the head's xl S2 (xm S1) alone --
    a wrong S2 or a swapped plane moves them by tens of percent; the bar is the suite's 1e-5."""
    from iago_amd import ops
    from tests.test_nets_shipped import TOL
    c = C.policy_head_case(piece)
    w1, b1, layers = _policy_args(c)
    own, opp = ops.bits_to_tensor(c["own"]), ops.bits_to_tensor(c["opp"])
    got = ops.policy_forward_split3(own, opp, w1, b1, layers, _dev(c["w9"]), _dev(c["b10"])).cpu().numpy()
    spread = c["probs"].max(axis=1) / c["probs"].min(axis=1)
    assert np.all(spread[[0, 1, 2, 3, 4]] > 1.2)          # the reachable positions hold all three cell states
    err = np.max(np.abs(got.astype(np.float64) - c["probs"]))
    assert err < TOL, err
