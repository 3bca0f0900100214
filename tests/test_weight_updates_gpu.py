"""Weights that change between launches, module by module: the GPU paths of SLPolicy and Value read forms cached
from the parameters (split / three-piece / float32-kernel / transposed weight pieces, the three-piece argument
template, the Value head's MFMA operand), each keyed by its tensors' (data_ptr, _version).  After every change
each path must give, bit for bit, what the same path gives on a module built fresh from the new weights
(`network.X().cuda().eval().load_npz(m.npz_dict())` -- no copy of the caches), and where a float64 restatement
exists stay within the shipped-net tolerance of it.  Every test warms the caches first and checks that they
hold entries, so that a stale entry would be read.

Changes: every parameter tensor in place, one at a time; Adam (fused launch and multi-tensor path); load_npz;
load_state_dict; a tensor's storage replaced (`p.data = ...`, which keeps its version); a .cpu() / .cuda()
round trip with the change made on the CPU."""
import os

import numpy as np
import pytest
import torch

from tests.conftest import GOLDEN, load_json
from tests.gpu_util import delta, fresh, random_positions

pytestmark = pytest.mark.gpu

TOL = 1e-5      # the shipped nets' tolerance to float64 (tests/test_nets_shipped.py), probabilities and values
N_REF = 6       # rows of each path checked against float64
POLICY_NAMES = ["block%d.conv.%s" % (k, w) for k in range(1, 9) for w in ("weight", "bias")] + ["conv9.weight",
                                                                                               "bias10.b"]
VALUE_NAMES = ["block%d.conv.%s" % (k, w) for k in range(1, 10) for w in ("weight", "bias")] + ["fc10.weight",
                                                                                               "fc11.weight"]


def _shipped(kind):
    from iago_amd import network
    cls, f = (network.SLPolicy, "sl_model.npz") if kind == "policy" else (network.Value, "value_model.npz")
    return cls().load_npz(os.path.join(GOLDEN, f)).cuda().eval()


@pytest.fixture(scope="module")
def boards():
    from iago_amd import ops
    own, opp = random_positions(320, seed=61)
    o, p = ops.bits_to_tensor(own), ops.bits_to_tensor(opp)
    g = torch.Generator().manual_seed(7)
    w = load_json("simulate.json")
    return dict(own=o, opp=p, planes=ops.encode_planes(o, p), np_planes=ops.encode_planes(o, p).cpu().numpy(),
                index=torch.randperm(64, generator=g).cuda(), index256=torch.randperm(256, generator=g).cuda(),
                action=torch.randint(0, 64, (48,), generator=g).to(torch.int32).cuda(),
                reward=(torch.randint(0, 2, (48,), generator=g) * 2 - 1).to(torch.float32).cuda(),
                result=(torch.rand(48, generator=g) * 2 - 1).cuda(),
                hc=torch.tensor([0, 1 << 20] * 4, dtype=torch.int64, device="cuda"),
                rw=ops.RolloutWeights(w["shipped_w"], w["shipped_b"]))


# -- the paths ------------------------------------------------------------------------------------------------------

def policy_paths(m, B):
    """Every GPU inference path of an SLPolicy: name -> output (device tensors).  (name, rows of np_planes) of the
    rows each output has in float64 go to policy_refs."""
    from iago_amd import rl_self_play
    x, o, p, idx = B["planes"], B["own"], B["opp"], B["index"]
    k = 37
    n_dev = torch.tensor([k], dtype=torch.int32, device="cuda")
    out = {}
    with torch.no_grad():
        for n in (5, 100, 300):
            assert m._use_f32_kernels(x[:n]) == (n <= m.F32_MAX_BATCH)
            out["forward%d" % n] = m(x[:n]).clone()
        out["counted"] = m.forward_counted(x[:64], n_dev)[:k].clone()
        for s3 in (True, False):
            m.split3 = s3
            try:
                out["boards_split3=%d" % s3] = m.forward_counted_boards(o, p, idx, 64, n_dev)[:k].clone()
            finally:
                del m.split3
    r = rl_self_play.play_batch(m, m, 8, handicap=B["hc"], seed=5, game_id_base=40)
    for name in ("own", "opp", "action", "z", "final_p1", "final_p2"):
        out["play_" + name] = r[name].clone()
    out["play_turns"] = torch.tensor([r["n_turns"]])
    return out


def policy_refs(B):
    rows = np.arange(N_REF)
    by_index = B["index"][:N_REF].cpu().numpy()
    return {"forward5": rows[:5], "forward100": rows, "forward300": rows, "counted": rows,
            "boards_split3=1": by_index, "boards_split3=0": by_index}


def value_paths(m, B):
    """Every GPU inference path of a Value net: name -> output."""
    from iago_amd import ops
    x, o, p = B["planes"], B["own"][:256], B["opp"][:256]
    n_dev = torch.tensor([200], dtype=torch.int32, device="cuda")
    out = {}
    with torch.no_grad():
        assert not m._use_split(x[:64])
        out["forward64"] = m(x[:64]).clone()
        for fused in (True, False):
            m.fused = fused
            try:
                assert m._use_split(x[:256])
                out["forward256_fused=%d" % fused] = m(x[:256]).clone()
                out["boards_fused=%d" % fused] = m.forward_boards(o, p).clone()
            finally:
                del m.fused
        ob = torch.full((256,), 9.0, dtype=torch.float32, device="cuda")
        m.forward_boards_batch(o, p, n_dev, ob, 2, 48)
        out["batch"] = ob
        ov = torch.full((256,), -77.0, dtype=torch.float32, device="cuda")
        res = ops.RolloutResult()
        ro = ops.rollout_prepare(o, p, B["rw"], seed=11, id_base=3000, stream_id=2, want_final=True, want_turns=True,
                                 out=res)
        m.forward_boards_counted(o, p, B["index256"], n_dev, ov, rollout=ro)
        out["value_rollout"], out["rollout_z"] = ov, res.z.clone()
    return out


def value_refs(B):
    rows = np.arange(N_REF)
    return {"forward64": rows, "forward256_fused=1": rows, "forward256_fused=0": rows, "boards_fused=1": rows,
            "boards_fused=0": rows, "batch": rows, "value_rollout": B["index256"][:N_REF].cpu().numpy()}


def grads(m, B):
    """reinforce_grads / value_grads on 48 rows: the loss and every parameter's gradient."""
    o, p = B["own"][:48], B["opp"][:48]
    if hasattr(m, "reinforce_grads"):
        loss = m.reinforce_grads(o, p, B["action"], B["reward"])
    else:
        loss = m.value_grads(o, p, B["result"])
    out = {"loss": loss.clone()}
    out.update({"grad " + n: q.grad.clone() for n, q in m.named_parameters()})
    return out


def run_all(m, B):
    out = policy_paths(m, B) if hasattr(m, "split3") else value_paths(m, B)
    out.update(grads(m, B))
    return out


def warm(m, B):
    """All paths once; the caches they read now hold entries."""
    out = run_all(m, B)
    d = m.__dict__
    assert set(d["_f32_cache"]) == set(range(2, 9))
    assert "_bwd_cache" in d
    if hasattr(m, "split3"):
        assert d["_split3_cache"][2] is not None            # the layers and the argument template (key2)
    else:
        assert set(d["_split_cache"]) == set(range(2, 9)) and "_head_cache" in d
    return out


def float64_outputs(m, x):
    """The net with m's weights in float64 (torch on the CPU, as tests/test_nets_shipped.py): probabilities for an
    SLPolicy, values for a Value net, of the planes x."""
    m64 = type(m)().double().eval().load_npz(m.npz_dict())
    with torch.no_grad():
        return m64(torch.from_numpy(x).double()).numpy()


def assert_follows(m, B, before, min_move=10 * TOL):
    """m's paths now give bit for bit what a freshly built module on m's weights gives, are within TOL of float64 on
    those weights, and the float outputs moved (by more than min_move on the float64-checked rows)."""
    got = run_all(m, B)
    want = run_all(fresh(m), B)
    assert set(got) == set(want)
    for k in got:
        assert torch.equal(got[k], want[k]), "%s differs from a freshly built module's" % k
    policy = hasattr(m, "split3")
    refs = policy_refs(B) if policy else value_refs(B)
    # the float64 reference ONCE, on the distinct rows the paths are checked on
    rows_all = np.unique(np.concatenate(list(refs.values())))
    ref_all = float64_outputs(m, B["np_planes"][rows_all])
    moved = 0.0
    for k, rows in refs.items():
        ref = ref_all[np.searchsorted(rows_all, rows)]
        out = got[k].cpu().numpy()
        out = out[rows] if k == "value_rollout" else out[:len(rows)]
        err = np.max(np.abs(out - ref))
        assert err < TOL, (k, err)
        old = before[k].cpu().numpy()
        old = old[rows] if k == "value_rollout" else old[:len(rows)]
        moved = max(moved, float(np.max(np.abs(out - old))))
    assert moved > min_move, moved
    if min_move >= TOL:
        for k in refs:
            assert not torch.equal(got[k], before[k]), "%s did not change" % k
    return got


# -- every tensor, in place -------------------------------------------------------------------------------------------

# (SLPolicy block8's bias reaches the distribution only through the cells where block8's ReLU is off -- elsewhere it
# shifts every logit alike, which the softmax cancels: it moves the shipped net's outputs by ~1e-7)
_FAINT = {("policy", "block8.conv.bias"): 1e-8}


@pytest.mark.parametrize("kind,name", [("policy", n) for n in POLICY_NAMES] + [("value", n) for n in VALUE_NAMES])
def test_every_tensor_changed_in_place(boards, kind, name):
    m = _shipped(kind)
    before = warm(m, boards)
    p = dict(m.named_parameters())[name]
    with torch.no_grad():
        p.add_(delta(p, seed=len(name)))
    assert_follows(m, boards, before, min_move=_FAINT.get((kind, name), 10 * TOL))


# -- how the weights change -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["policy", "value"])
@pytest.mark.parametrize("native", [True, False])
def test_adam_update(boards, kind, native, monkeypatch):
    """ChainerAdam.update on the gradients of the kernels: its fused launch (iago_adam_chainer, the subtraction as a
    multi-tensor op) and its multi-tensor path."""
    from iago_amd import train_rl
    monkeypatch.setattr(train_rl, "NATIVE_GRAD", native)
    m = _shipped(kind)
    before = warm(m, boards)           # (leaves every .grad set)
    opt = train_rl.ChainerAdam(m)
    opt.update()
    assert not native or "_steps" in opt.__dict__
    assert_follows(m, boards, before)


def _other_weights(m):
    return {k: v + delta(torch.from_numpy(v), seed=i).numpy() for i, (k, v) in enumerate(sorted(m.npz_dict().items()))}


@pytest.mark.parametrize("kind", ["policy", "value"])
def test_load_npz(boards, kind):
    m = _shipped(kind)
    before = warm(m, boards)
    other = _other_weights(m)
    m.load_npz(other)
    assert all(np.array_equal(m.npz_dict()[k], other[k]) for k in other)
    assert_follows(m, boards, before)


@pytest.mark.parametrize("kind", ["policy", "value"])
def test_load_state_dict(boards, kind):
    m = _shipped(kind)
    before = warm(m, boards)
    sd = {k: v.clone() + delta(v, seed=i) for i, (k, v) in enumerate(m.state_dict().items())}
    m.load_state_dict(sd)
    assert_follows(m, boards, before)


@pytest.mark.parametrize("kind,names", [
    ("policy", ["block1.conv.weight"]), ("policy", ["conv9.weight", "bias10.b"]), ("policy", ["block1.conv.bias"]),
    ("policy", ["block5.conv.bias"]), ("policy", ["block3.conv.weight"]),
    ("value", ["block9.conv.weight"]), ("value", ["block4.conv.bias"]), ("value", ["block6.conv.weight"]),
    ("value", ["fc10.weight", "fc11.weight"])])
def test_storage_replaced(boards, kind, names):
    """`p.data = new tensor`: the parameter's version does not change, its storage does (the caches that hold a
    tensor itself must tell by its pointer)."""
    m = _shipped(kind)
    before = warm(m, boards)
    params = dict(m.named_parameters())
    v0 = [params[n]._version for n in names]
    for i, n in enumerate(names):
        params[n].data = params[n].data + delta(params[n], seed=i + 3)
    assert [params[n]._version for n in names] == v0
    assert_follows(m, boards, before)


@pytest.mark.parametrize("kind,names", [("policy", ["block1.conv.weight"]), ("policy", ["block4.conv.bias"]),
                                        ("policy", ["bias10.b"]), ("value", ["block9.conv.weight"]),
                                        ("value", ["block2.conv.weight", "fc11.weight"])])
def test_round_trip_through_the_cpu(boards, kind, names):
    """.cpu(), the change made there, .cuda(): new storages on the device (possibly at the addresses the old ones
    had) with the versions the CPU change gave them."""
    m = _shipped(kind)
    before = warm(m, boards)
    m.cpu()
    params = dict(m.named_parameters())
    with torch.no_grad():
        for i, n in enumerate(names):
            params[n].add_(delta(params[n], seed=i + 5))
    m.cuda()
    assert all(q.is_cuda for q in m.parameters())
    assert_follows(m, boards, before)
