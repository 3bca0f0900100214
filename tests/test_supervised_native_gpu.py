"""SupervisedTrainer(native=True): the supervised updates of train_value.py / train_policy.py with their gradients from
the split-f16 kernels (Value.value_grads, SLPolicy.reinforce_grads) and Chainer's Adam."""
import copy
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
SCALE = float(np.float32(1.0 / (1.0 - 0.4)))


def _rows(n, seed):
    """n positions from policy-vs-policy games (own = the side to move), their moves and results."""
    from iago_amd import network, rl_self_play
    torch.manual_seed(seed)
    m = network.SLPolicy().cuda().eval()
    r = rl_self_play.play_batch(m, m, 64, seed=seed)
    valid = r["action"] >= 0
    z = r["z"].reshape(1, -1).expand_as(r["action"])
    own, opp, act, zz = r["own"][valid], r["opp"][valid], r["action"][valid], z[valid].to(torch.float32)
    reps = (n + own.numel() - 1) // own.numel()
    return [t.repeat(reps)[:n].contiguous() for t in (own, opp, act, zz)]


def _trunk_masks(model, own, opp, layers):
    """[x_k > 0] of blocks 1..8 as the split-f16 forward computes them."""
    from iago_amd import ops
    a = ops.value_stem_boards(own, opp, model.block1.conv.weight.detach(), model.block1.conv.bias.detach())
    masks = [ops.merge_nchw(a) > 0]
    for hi, lo, bias in layers:
        a = ops.conv3x3_split(a, hi, lo, bias)
        masks.append(ops.merge_nchw(a) > 0)
    return masks


def _value_h9(model, own, opp, y):
    """Block 9's output as the update's kernels compute it (its ReLU decisions)."""
    from iago_amd import network, ops
    n = own.numel()
    h9 = torch.empty(n, 64, device="cuda")
    layers = [model._split_weights(k) + (getattr(model, "block%d" % k).conv.bias.detach(),) for k in range(2, 9)]
    g = {k: torch.empty_like(p) for k, p in model.named_parameters()}
    grads = dict(w1=g["block1.conv.weight"], b1=g["block1.conv.bias"],
                 w=[g["block%d.conv.weight" % k] for k in range(2, 9)], b=[g["block%d.conv.bias" % k] for k in range(2, 9)],
                 w9=g["block9.conv.weight"], b9=g["block9.conv.bias"], w10=g["fc10.weight"], w11=g["fc11.weight"])
    ops.value_mse_grad(own, opp, y, n, model.block1.conv.weight.detach(), model.block1.conv.bias.detach(), layers,
                       network._bwd_layers(model), model.block9.conv.weight.detach(), model.block9.conv.bias.detach(),
                       model.fc10.weight.detach(), model.fc11.weight.detach(), grads, h9=h9)
    return h9, layers


def _value_grads64(model, own, opp, y, keep):
    """float64 autograd of train_value.py:53-57 with the split-f16 forward's ReLU decisions and the given mask."""
    from iago_amd import ops
    h9k, layers = _value_h9(model, own, opp, y)
    masks = _trunk_masks(model, own, opp, layers)
    m = copy.deepcopy(model).double().train()
    h = ops.encode_planes(own, opp).double()
    for k in range(1, 9):
        h = getattr(m, "block%d" % k).conv(h) * masks[k - 1]
    pre9 = m.block9.conv(h).reshape(-1, 64) * (h9k > 0)
    pred = m.fc11(m.fc10(pre9) * (keep.double() * SCALE)).reshape(-1)
    torch.sum((pred - y.double()) ** 2).div(own.numel()).backward()
    return {k: p.grad for k, p in m.named_parameters()}


def _adam64(p, g, m, v, t, delta):
    """One step of Chainer's Adam + WeightDecay(5e-4) in float64, and how far the parameter can move when every
    gradient entry moves by up to `delta` (Adam divides by the gradient's own size: small entries amplify errors)."""
    a_t = 1e-3 * math.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t)

    def step(gg):
        g2 = gg + 5e-4 * p
        m2 = m + 0.1 * (g2 - m)
        v2 = v + 0.001 * (g2 * g2 - v)
        return p - a_t * m2 / (torch.sqrt(v2) + 1e-8)

    center = step(g)
    tol = torch.zeros_like(p)
    for s in (-1.0, -0.5, 0.5, 1.0):
        tol = torch.maximum(tol, (step(g + s * delta) - center).abs())
    return center, tol


def _record_updates(tr):
    """Wrap tr.opt.update: the parameters, moments and step count before each step, the parameters after."""
    log = []
    real = tr.opt.update

    def update():
        before = {n: (p.detach().double().clone(), tr.opt.state[n][0].double().clone(),
                      tr.opt.state[n][1].double().clone(), p.grad.clone()) for n, p in tr.model.named_parameters()}
        real()
        after = {n: p.detach().double().clone() for n, p in tr.model.named_parameters()}
        log.append((tr.opt.t, before, after))
    tr.opt.update = update
    return log


def test_native_value_steps_match_float64_adam():
    """Two native minibatches of one epoch (4,096 + 500 rows): replaying the trainer's documented draws (the epoch's
    permutation, then per minibatch its (m, 128) mask), every step equals one Adam step from float64-autograd
    gradients at the parameters it started from -- the second one proves the cached weight layouts follow Adam."""
    from iago_amd import network
    from iago_amd.train_supervised import MINIBATCH, SupervisedTrainer
    n, seed = MINIBATCH + 500, 17
    own, opp, _, y = _rows(n, seed=2)
    torch.manual_seed(4)
    model = network.Value().cuda()
    tr = SupervisedTrainer(model, "value", seed=seed, native=True)
    log = _record_updates(tr)
    tr.epoch(own, opp, y)
    assert tr.opt.t == 2 and len(log) == 2
    gen = torch.Generator(device="cuda").manual_seed(seed)
    perm = torch.randperm(n, device="cuda", generator=gen)
    probe = network.Value().cuda()
    for step, lo in enumerate(range(0, n, MINIBATCH)):
        idx = perm[lo:lo + MINIBATCH]
        keep = torch.rand((idx.numel(), 128), device="cuda", generator=gen) >= 0.4
        t, before, after = log[step]
        with torch.no_grad():
            for name, p in probe.named_parameters():
                p.copy_(before[name][0])
        ref = _value_grads64(probe, own[idx], opp[idx], y[idx], keep)
        for name in ref:
            p0, m0, v0, g_native = before[name]
            assert float((g_native.double() - ref[name]).abs().max()) <= 1e-5 * float(ref[name].abs().max()), \
                (step, name)
            want, tol = _adam64(p0, ref[name], m0, v0, t, 2e-5 * float(ref[name].abs().max()))
            err = (after[name] - want).abs()
            bound = tol + 2.0 ** -22 * p0.abs() + 1e-9
            assert bool((err <= bound).all()), (step, name, float((err - bound).max()))


def test_native_policy_gradients_equal_autograd_policy_loss():
    """SLPolicy + 'policy': the gradients of mean(softmax_cross_entropy(model(x), y)) (train_policy.py:59-61) through
    iago_policy_reinforce_grad with every reward 1, against float64 autograd of policy_loss's arithmetic."""
    from iago_amd import network, ops
    from iago_amd.train_supervised import SupervisedTrainer
    own, opp, act, _ = _rows(1200, seed=6)
    torch.manual_seed(8)
    model = network.SLPolicy().cuda()
    probe = copy.deepcopy(model)
    tr = SupervisedTrainer(model, "policy", seed=2, native=True)
    log = _record_updates(tr)
    tr.epoch(own, opp, act)
    assert len(log) == 1
    layers = [(hi, mid, bias) for hi, mid, lo, bias in probe._split3_layers()]
    masks = _trunk_masks(probe, own, opp, layers)
    m64 = copy.deepcopy(probe).double().train()
    h = ops.encode_planes(own, opp).double()
    for k in range(1, 9):
        h = getattr(m64, "block%d" % k).conv(h) * masks[k - 1]
    pred = torch.softmax(m64.bias10(m64.conv9(h).reshape(-1, 64)), dim=1)
    F.cross_entropy(pred, act.to(torch.int64)).backward()          # policy_loss's loss on the model's output
    _, before, _ = log[0]
    for name, p in m64.named_parameters():
        got = before[name][3].double()
        assert float((got - p.grad).abs().max()) <= 1e-5 * float(p.grad.abs().max()), name


def test_native_value_training_end_to_end(tmp_path):
    """value_self_play data (the shipped SL net for both phases, 4,096 games) -> 8-fold augmentation -> 3 native epochs
    from the shipped Value net: the loss falls epoch by epoch and on the whole set, Adam counts the minibatches, and the
    epochs' losses follow autograd's from the same start; the saved net drives a search without saturating.  (The loss
    on held-out games is no criterion at this size: measured, both arms overfit 4,096 games from the shipped net, and a
    random-init net stays at E[z^2] in both for ten epochs.)"""
    from iago_amd import engine, network, ops, value_self_play
    from iago_amd.train_supervised import MINIBATCH, SupervisedTrainer
    sl = network.SLPolicy().load_npz(os.path.join(GOLDEN, "sl_model.npz")).cuda().eval()
    r = value_self_play.generate(sl, sl, 4096, seed=1)
    keep = ~r["dropped"]
    own, opp, z = r["own"][keep].contiguous(), r["opp"][keep].contiguous(), r["z"][keep].to(torch.float32)
    oo, po, _ = ops.augment8(own, opp, torch.zeros(own.numel(), dtype=torch.int8, device="cuda"))
    own, opp, z = oo.reshape(-1).contiguous(), po.reshape(-1).contiguous(), z.repeat(8).contiguous()
    start = network.Value().load_npz(os.path.join(GOLDEN, "value_model.npz")).cuda()
    model = copy.deepcopy(start)
    tr = SupervisedTrainer(model, "value", seed=3, native=True)
    first = tr.evaluate(own, opp, z)["loss"]
    losses = [tr.epoch(own, opp, z) for _ in range(3)]
    last = tr.evaluate(own, opp, z)["loss"]
    ref = SupervisedTrainer(copy.deepcopy(start), "value", seed=3)
    ref_losses = [ref.epoch(own, opp, z) for _ in range(3)]
    print("value training: loss %.4f -> %.4f, epochs %s (autograd %s)" % (first, last, losses, ref_losses))
    assert losses[0] > losses[1] > losses[2] and last < first
    for a, b in zip(losses, ref_losses):
        assert abs(a - b) <= 0.01 * b
    assert tr.opt.t == 3 * ((own.numel() + MINIBATCH - 1) // MINIBATCH)
    path = str(tmp_path / "value.npz")
    model.save_npz(path)
    v2 = network.Value().load_npz(path).cuda().eval()
    for (k, a), b in zip(model.named_parameters(), v2.parameters()):
        assert torch.equal(a.detach(), b.detach()), k
    G = 32
    m = engine.BatchedMCTS(G, sl, v2, ops.uniform_weights(), n_thr=15, capacity=engine.suggest_capacity(64, 15),
                           seed=3)
    o = torch.full((G,), engine.START_OWN, dtype=torch.int64, device="cuda")
    p = torch.full((G,), engine.START_OPP, dtype=torch.int64, device="cuda")
    m.search(o, p, torch.ones(G, dtype=torch.uint8, device="cuda"), 64)
    v2.check_saturation()
    sl.check_saturation()


def test_native_refuses_other_models():
    from iago_amd import network
    from iago_amd.train_supervised import SupervisedTrainer
    with pytest.raises(ValueError):
        SupervisedTrainer(network.RolloutPolicy(), "policy", native=True)
    with pytest.raises(ValueError):
        SupervisedTrainer(network.Value(), "policy", native=True)
    v = network.Value()
    v.split_f16 = False
    with pytest.raises(ValueError):
        SupervisedTrainer(v, "value", native=True)
    v2 = network.Value()
    v2.split_f16 = False
    with pytest.raises(ValueError):
        v2.cuda().value_grads(torch.zeros(4, dtype=torch.int64, device="cuda"),
                              torch.zeros(4, dtype=torch.int64, device="cuda"), torch.zeros(4, device="cuda"))
