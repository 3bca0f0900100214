"""The Value net's supervised gradients on the split-f16 kernels (iago_value_mse_grad, csrc/policy_grad_kernels.hip)
against float64 autograd of the reference's loss (train_value.py:53-57: pred = model(x), loss =
mean_squared_error(pred, y), backward)."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
SCALE = float(np.float32(1.0 / (1.0 - 0.4)))


def rel_err(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def _rows(n, seed):
    """n positions from real policy-vs-policy games (own = the side to move) and a result in {-1, 1} for each, in a
    shuffled order (the games' first plies are 64 copies of the opening: a few rows of one board whose results cancel
    make a gradient that is nearly zero against its terms, and no arithmetic keeps its relative digits there)."""
    from iago_amd import network, rl_self_play
    torch.manual_seed(seed)
    m = network.SLPolicy().cuda().eval()
    r = rl_self_play.play_batch(m, m, 64, seed=seed)
    valid = r["action"] >= 0
    z = r["z"].reshape(1, -1).expand_as(r["action"])
    own, opp, zz = r["own"][valid], r["opp"][valid], z[valid].to(torch.float32)
    order = torch.randperm(own.numel(), generator=torch.Generator().manual_seed(seed)).to(own.device)
    own, opp, zz = own[order], opp[order], zz[order]
    reps = (n + own.numel() - 1) // own.numel()
    return [t.repeat(reps)[:n].contiguous() for t in (own, opp, zz)]


def _relu_masks(model, own, opp):
    """[x_k > 0] of blocks 1..8 as the split-f16 forward computes them (the same kernels as the update's forward)."""
    from iago_amd import ops
    a = ops.value_stem_boards(own, opp, model.block1.conv.weight.detach(), model.block1.conv.bias.detach())
    masks = [ops.merge_nchw(a) > 0]
    for k in range(2, 9):
        hi, lo = model._split_weights(k)
        a = ops.conv3x3_split(a, hi, lo, getattr(model, "block%d" % k).conv.bias.detach())
        masks.append(ops.merge_nchw(a) > 0)
    return masks


def _autograd(model, own, opp, y, keep=None, masks=None, h9=None, dtype=torch.float64, n_mean=None):
    """The reference's loss and gradients by autograd in `dtype`.  masks / h9: the ReLU decisions of blocks 1..8 and
    of block 9 taken from there instead of from the pre-activations of this arithmetic (a pre-activation within
    rounding of zero flips a ReLU between two arithmetics, and one flipped cell moves a weight gradient -- a sum of
    cancelling terms -- by far more than the rounding).  keep: fc10's dropout mask, kept units times 1 / (1 - 0.4)."""
    from iago_amd import ops
    m = copy.deepcopy(model).to(dtype).train()
    for p in m.parameters():
        p.grad = None
    h = ops.encode_planes(own, opp).to(dtype)
    for k in range(1, 9):
        pre = getattr(m, "block%d" % k).conv(h)
        h = torch.relu(pre) if masks is None else pre * masks[k - 1]
    pre9 = m.block9.conv(h).reshape(-1, 64)
    h9v = torch.relu(pre9) if h9 is None else pre9 * (h9 > 0)
    h10 = m.fc10(h9v)
    if keep is not None:
        h10 = h10 * (keep.to(dtype) * SCALE)
    pred = m.fc11(h10).reshape(-1)
    loss = torch.sum((pred - y.to(dtype)) ** 2) / (own.numel() if n_mean is None else n_mean)
    loss.backward()
    return loss.detach(), {k: p.grad for k, p in m.named_parameters()}


def _native(model, own, opp, y, keep=None):
    """Value.value_grads + the kernel's h9 (block 9's ReLU decisions) from the ops-level call on the same weights."""
    from iago_amd import network, ops
    n = own.numel()
    h9 = torch.empty(n, 64, device="cuda")
    layers = [model._split_weights(k) + (getattr(model, "block%d" % k).conv.bias.detach(),) for k in range(2, 9)]
    scratch = {k: torch.empty_like(p) for k, p in model.named_parameters()}
    grads = dict(w1=scratch["block1.conv.weight"], b1=scratch["block1.conv.bias"],
                 w=[scratch["block%d.conv.weight" % k] for k in range(2, 9)],
                 b=[scratch["block%d.conv.bias" % k] for k in range(2, 9)],
                 w9=scratch["block9.conv.weight"], b9=scratch["block9.conv.bias"],
                 w10=scratch["fc10.weight"], w11=scratch["fc11.weight"])
    ops.value_mse_grad(own, opp, y, n, model.block1.conv.weight.detach(), model.block1.conv.bias.detach(), layers,
                       network._bwd_layers(model), model.block9.conv.weight.detach(), model.block9.conv.bias.detach(),
                       model.fc10.weight.detach(), model.fc11.weight.detach(), grads,
                       keep=None if keep is None else keep.to(torch.uint8), h9=h9)
    loss = model.value_grads(own, opp, y, keep=keep)
    got = {k: p.grad.clone() for k, p in model.named_parameters()}
    for k in got:                                   # (the two calls: the same kernels on the same data)
        assert torch.equal(got[k], scratch[k]), k
    return loss, got, h9


def _keep(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand((n, 128), device="cuda", generator=g) >= 0.4


@pytest.mark.parametrize("n", [1, 5, 70, 1900, 4096])
@pytest.mark.parametrize("dropout", [True, False])
def test_value_gradients_against_float64_autograd(n, dropout):
    from iago_amd import network
    own, opp, y = _rows(n, seed=n)
    torch.manual_seed(3 + n)
    model = network.Value().cuda()
    keep = _keep(n, n) if dropout else None
    loss, got, h9 = _native(model, own, opp, y, keep)
    assert int(model._overflow_flag(own.device).item()) == 0
    loss64, ref = _autograd(model, own, opp, y, keep, masks=_relu_masks(model, own, opp), h9=h9)
    assert abs(float(loss) - float(loss64)) <= 1e-6 * abs(float(loss64)), (float(loss), float(loss64))
    worst = {k: rel_err(got[k], ref[k]) for k in ref if float(ref[k].abs().max()) > 0}
    print("n = %d, dropout %s: worst tensor %s %.2e" % ((n, dropout) + max(worst.items(), key=lambda kv: kv[1])))
    for k, e in worst.items():
        assert e < 1e-5, (k, e)


@pytest.mark.parametrize("dropout", [True, False])
def test_shipped_value_net_gradients(dropout):
    """The shipped net: tensor by tensor the kernels must be as close to float64 as float32 autograd is."""
    from iago_amd import network
    n = 1900
    own, opp, y = _rows(n, seed=21)
    model = network.Value().load_npz(os.path.join(GOLDEN, "value_model.npz")).cuda()
    keep = _keep(n, 5) if dropout else None
    loss, got, h9 = _native(model, own, opp, y, keep)
    assert int(model._overflow_flag(own.device).item()) == 0
    loss64, ref = _autograd(model, own, opp, y, keep, masks=_relu_masks(model, own, opp), h9=h9)
    _, plain = _autograd(model, own, opp, y, keep)
    _, got32 = _autograd(model, own, opp, y, keep, dtype=torch.float32)
    assert abs(float(loss) - float(loss64)) <= 1e-6 * abs(float(loss64))
    top = max(float(ref[k].abs().max()) for k in ref)
    for k in ref:
        scale = float(ref[k].abs().max())
        if scale < 1e-4 * top:
            continue        # (a tensor that cancels to nothing)
        mine = float((got[k].double() - ref[k]).abs().max()) / scale
        theirs = float((got32[k].double() - plain[k]).abs().max()) / float(plain[k].abs().max())
        print("%s: split-f16 %.2e, float32 autograd %.2e" % (k, mine, theirs))
        assert mine <= max(10 * theirs, 1e-5) and mine < 1e-3, (k, mine, theirs)


def test_pred_equals_inference():
    """keep=None: the model's output is the split-f16 inference's (Value.eval() on the same boards)."""
    from iago_amd import network
    n = 1900
    own, opp, y = _rows(n, seed=8)
    model = network.Value().load_npz(os.path.join(GOLDEN, "value_model.npz")).cuda()
    pred = torch.empty(n, device="cuda")
    model.value_grads(own, opp, y, pred=pred)
    model.eval()
    with torch.no_grad():
        want = model.forward_boards(own, opp)
    assert want is not None
    assert float((pred - want).abs().max()) <= 1e-6 * max(1.0, float(want.abs().max()))


def test_value_gradients_are_deterministic():
    from iago_amd import network
    own, opp, y = _rows(1500, seed=3)
    torch.manual_seed(9)
    model = network.Value().cuda()
    keep = _keep(1500, 1)
    runs = []
    for _ in range(3):
        loss = model.value_grads(own, opp, y, keep=keep)
        runs.append([float(loss)] + [p.grad.clone() for p in model.parameters()])
        torch.empty(1 << 26, device="cuda").normal_()        # (other bytes where freed scratch may have been)
    for other in runs[1:]:
        assert other[0] == runs[0][0]
        for a, b in zip(runs[0][1:], other[1:]):
            assert torch.equal(a, b)


def test_rows_in_chunks_give_the_one_call_gradients(monkeypatch):
    from iago_amd import network
    own, opp, y = _rows(700, seed=11)
    torch.manual_seed(3)
    model = network.Value().cuda()
    keep = _keep(700, 2)
    loss1 = model.value_grads(own, opp, y, keep=keep)
    one = {k: p.grad.clone() for k, p in model.named_parameters()}
    monkeypatch.setattr(network.Value, "GRAD_CHUNK_ROWS", 256)
    pred = torch.full((700,), float("nan"), device="cuda")
    loss3 = model.value_grads(own, opp, y, keep=keep, pred=pred)
    three = {k: p.grad.clone() for k, p in model.named_parameters()}
    assert abs(float(loss1) - float(loss3)) <= 1e-6 * abs(float(loss1))
    for k in one:
        assert rel_err(three[k], one[k]) < 1e-6, (k, rel_err(three[k], one[k]))
    assert bool(torch.isfinite(pred).all())                                          # every chunk wrote its rows


def test_saturation_raises_the_flag_and_the_native_trainer_applies_nothing():
    from iago_amd import _lib, network
    from iago_amd.train_supervised import SupervisedTrainer
    own, opp, y = _rows(300, seed=4)
    torch.manual_seed(6)
    model = network.Value().cuda()
    with torch.no_grad():
        model.block2.conv.weight.mul_(1e6)
    model.value_grads(own, opp, y)
    flag = model._overflow_flag(own.device)
    assert int(flag.item()) & 1
    flag.zero_()
    tr = SupervisedTrainer(model, "value", seed=1, native=True)
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    with pytest.raises(_lib.IagoError):
        tr.epoch(own, opp, y)
    assert tr.opt.t == 0
    for k, p in model.named_parameters():
        assert torch.equal(p.detach(), before[k]), k
        m, v = tr.opt.state[k]
        assert not bool(m.any()) and not bool(v.any()), k
    assert int(flag.item()) == 0                          # (the trainer cleared the word it reported)


def _policy_rows(n, seed):
    from iago_amd import network, rl_self_play
    torch.manual_seed(seed)
    m = network.SLPolicy().cuda().eval()
    r = rl_self_play.play_batch(m, m, 64, seed=seed)
    valid = r["action"] >= 0
    z = r["z"].reshape(1, -1).expand_as(r["action"])
    own, opp, act, zz = r["own"][valid], r["opp"][valid], r["action"][valid], z[valid]
    reps = (n + own.numel() - 1) // own.numel()
    return [t.repeat(reps)[:n].contiguous() for t in (own, opp, act, zz)]


def test_policy_update_is_unchanged():
    """The trunk the two entry points share: iago_policy_reinforce_grad still matches float64 autograd of
    src/train_rl.py:61-65 on fixed rows."""
    from iago_amd import network, ops
    own, opp, act, z = _policy_rows(300, seed=12)
    torch.manual_seed(5)
    model = network.SLPolicy().cuda()
    a = ops.value_stem_boards(own, opp, model.block1.conv.weight.detach(), model.block1.conv.bias.detach())
    masks = [ops.merge_nchw(a) > 0]
    for (hi, mid, lo, bias) in model._split3_layers():
        a = ops.conv3x3_split(a, hi, mid, bias)
        masks.append(ops.merge_nchw(a) > 0)
    m64 = copy.deepcopy(model).double().train()
    h = ops.encode_planes(own, opp).double()
    for k in range(1, 9):
        h = getattr(m64, "block%d" % k).conv(h) * masks[k - 1]
    pred = torch.softmax(m64.bias10(m64.conv9(h).reshape(-1, 64)), dim=1)
    loss64 = torch.sum(F.cross_entropy(pred, act.to(torch.int64), reduction="none") * z.double()) / own.numel()
    loss64.backward()
    loss64 = loss64.detach()
    loss = model.reinforce_grads(own, opp, act, z)
    model.check_saturation()
    assert abs(float(loss) - float(loss64)) <= 1e-6 * max(1.0, abs(float(loss64)))
    ref = dict(m64.named_parameters())
    for k, p in model.named_parameters():
        assert rel_err(p.grad, ref[k].grad) < 1e-5, k
