"""Training SLPolicy on the search's visit counts on the GPU (iago_policy_visits_grad, SLPolicy.visits_grads,
ReinforceTrainer.step_from_tuples(target="visits")): the head kernel of csrc/policy_grad_kernels.hip and the trunk it
shares with the REINFORCE update against float64 autograd of train_rl.visits_loss_from_logits, and the trainer's step
on the tuples of a small exploring self-play."""
import copy

import numpy as np
import pytest
import torch

from tests.test_policy_grad_gpu import _relu_masks, _rows, rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pool():
    """Recorded positions of real policy-vs-policy games, played once: every test takes a prefix."""
    own, opp, act, z = _rows(1030, seed=7)
    return own, opp, act, z


def _take(pool, n):
    return [t[:n].contiguous() for t in pool]


def _visits(own, opp, seed):
    """Visit rows on the positions' legal moves: counts 0 .. 40 from a fixed generator, row 0 one-hot and row n // 2
    all zero where n >= 2 (a single row keeps a count on every legal cell), weights in [0.25, 2]."""
    from iago_amd import ops
    n = own.numel()
    legal = ops.legal_moves(own, opp)
    on = ((legal.reshape(-1, 1) >> torch.arange(64, device=legal.device)) & 1).to(torch.int32)
    assert bool((on.sum(dim=1) > 0).all())                       # (the mover of a recorded row had a move)
    g = torch.Generator().manual_seed(seed)
    counts = torch.randint(0, 41, (n, 64), generator=g, dtype=torch.int32).cuda() * on
    weight = (0.25 + 1.75 * torch.rand(n, generator=g)).cuda()
    if n >= 2:
        counts[0] = 0
        counts[0, int(on[0].argmax())] = 17
        counts[n // 2] = 0
    else:
        counts = counts.clamp(min=1) * on
    return counts.contiguous(), weight


def _autograd64(model, own, opp, visits, weight, masks, n_mean=None):
    """visits_loss_from_logits and its gradients in float64 autograd on a .double() copy of the model, every ReLU's
    on / off decision taken from `masks` (the split-f16 forward's: see test_policy_grad_gpu._autograd64)."""
    from iago_amd import ops
    from iago_amd.train_rl import visits_loss_from_logits
    m64 = copy.deepcopy(model).double().train()
    for p in m64.parameters():
        p.grad = None
    h = ops.encode_planes(own, opp).double()
    for k in range(1, 9):
        h = getattr(m64, "block%d" % k).conv(h) * masks[k - 1]
    logits = m64.bias10(m64.conv9(h).reshape(-1, 64))
    loss = visits_loss_from_logits(logits, visits, None if weight is None else weight.double(), n_mean=n_mean)
    loss.backward()
    return loss.detach(), {k: p.grad for k, p in m64.named_parameters()}


def _grads(model):
    return {k: p.grad.clone() for k, p in model.named_parameters()}


@pytest.mark.parametrize("n", [1, 5, 70, 1030])
def test_visits_gradients_against_float64_autograd(pool, n):
    """1030 rows: the grid-stride loop of 256 workgroups x 4 waves takes a second pass.  Bounds of
    test_policy_grad_gpu.py (the trunk kernels are the same)."""
    from iago_amd import network, train_rl
    own, opp, _, _ = _take(pool, n)
    visits, weight = _visits(own, opp, seed=100 + n)
    torch.manual_seed(5)
    model = network.SLPolicy().cuda()
    loss64, ref = _autograd64(model, own, opp, visits, weight, _relu_masks(model, own, opp))
    loss = model.visits_grads(own, opp, visits, weight)
    model.check_saturation()
    got = _grads(model)
    model.train()
    for p in model.parameters():
        p.grad = None
    train_rl.visits_loss(model, own, opp, visits, weight).backward()
    got32 = _grads(model)
    print("n = %d: loss %.9g against %.9g in float64" % (n, float(loss), float(loss64)))
    for k in ref:
        scale = float(ref[k].abs().max())
        mine = float((got[k].double() - ref[k]).abs().max()) / scale
        theirs = float((got32[k].double() - ref[k]).abs().max()) / scale
        print("  %-20s split-f16 %.2e, float32 autograd %.2e of the largest entry %.2e" % (k, mine, theirs, scale))
    assert abs(float(loss) - float(loss64)) <= 1e-6 * max(1.0, abs(float(loss64)))
    for k in ref:
        scale = float(ref[k].abs().max())
        mine = float((got[k].double() - ref[k]).abs().max()) / scale
        theirs = float((got32[k].double() - ref[k]).abs().max()) / scale
        assert mine < 1e-5, (k, mine)
        assert mine < max(10 * theirs, 1e-5), (k, mine, theirs)


def test_a_row_without_visits_contributes_nothing(pool):
    from iago_amd import network
    own, opp, _, _ = _take(pool, 71)
    visits, weight = _visits(own, opp, seed=21)
    visits[70] = 0
    torch.manual_seed(6)
    model = network.SLPolicy().cuda()
    loss70 = float(model.visits_grads(own[:70], opp[:70], visits[:70], weight[:70], n_mean=70))
    alone = _grads(model)
    loss71 = float(model.visits_grads(own, opp, visits, weight, n_mean=70))
    model.check_saturation()
    withrow = _grads(model)
    assert abs(loss70 - loss71) <= 1e-6 * max(1.0, abs(loss70))
    for k in alone:                                              # (the trunk's grouping follows n: not bit for bit)
        assert rel_err(withrow[k], alone[k]) < 2e-6, (k, rel_err(withrow[k], alone[k]))


def test_visits_gradients_are_deterministic(pool):
    from iago_amd import network
    own, opp, _, _ = _take(pool, 300)
    visits, weight = _visits(own, opp, seed=22)
    torch.manual_seed(9)
    model = network.SLPolicy().cuda()
    runs = []
    for _ in range(3):
        loss = model.visits_grads(own, opp, visits, weight)
        runs.append([float(loss)] + [p.grad.clone() for p in model.parameters()])
        torch.empty(1 << 26, device="cuda").normal_()            # (other bytes where freed scratch may have been)
    for other in runs[1:]:
        assert other[0] == runs[0][0]
        for a, b in zip(runs[0][1:], other[1:]):
            assert torch.equal(a, b)


def test_rows_in_chunks_give_the_one_call_gradients(pool, monkeypatch):
    from iago_amd import network
    own, opp, _, _ = _take(pool, 700)
    visits, weight = _visits(own, opp, seed=23)
    torch.manual_seed(3)
    model = network.SLPolicy().cuda()
    loss1 = float(model.visits_grads(own, opp, visits, weight))
    one = _grads(model)
    monkeypatch.setattr(network.SLPolicy, "GRAD_CHUNK_ROWS", 256)
    probs = torch.empty(700, 64, device="cuda")
    loss3 = float(model.visits_grads(own, opp, visits, weight, probs=probs))
    three = _grads(model)
    assert abs(loss1 - loss3) <= 1e-6 * max(1.0, abs(loss1))
    for k in one:
        assert rel_err(three[k], one[k]) < 2e-6, (k, rel_err(three[k], one[k]))
    assert float((probs.sum(dim=1) - 1).abs().max()) < 1e-5       # every chunk wrote its rows


def test_visits_of_the_wrong_kind_are_refused(pool):
    from iago_amd import network
    own, opp, _, _ = _take(pool, 5)
    visits, weight = _visits(own, opp, seed=24)
    model = network.SLPolicy().cuda()
    for bad in (visits.to(torch.int64), visits.float(), visits[:4], visits[:, :63], visits.reshape(-1)):
        with pytest.raises(ValueError):
            model.visits_grads(own, opp, bad)


def _tuples(own, opp, act, z, pi):
    n = own.numel()
    return dict(own=own, opp=opp, move=act.to(torch.int8), z=z.to(torch.int8), pi=pi,
                colour=torch.ones(n, dtype=torch.int8, device="cuda"),
                game=torch.zeros(n, dtype=torch.int32, device="cuda"),
                turn=torch.arange(n, dtype=torch.int32, device="cuda"))


def test_a_negative_count_raises_the_flag_and_the_trainer_applies_nothing(pool):
    from iago_amd import network, _lib
    from iago_amd.train_rl import ReinforceTrainer
    own, opp, act, z = _take(pool, 40)
    visits, weight = _visits(own, opp, seed=25)
    torch.manual_seed(4)
    model = network.SLPolicy().cuda()
    model.visits_grads(own, opp, visits, weight)
    assert int(model._overflow_flag(own.device).item()) == 0
    bad = visits.clone()
    bad[7, 33] = -1
    model.visits_grads(own, opp, bad, weight)
    assert int(model._overflow_flag(own.device).item()) & 2
    model._overflow_flag(own.device).zero_()
    tr = ReinforceTrainer(model, pool_dir=None, N=2, seed=1)
    before = {k: v.copy() for k, v in model.npz_dict().items()}
    with pytest.raises(_lib.IagoError, match="negative"):
        tr.step_from_tuples(_tuples(own, opp, act, z, bad), target="visits")
    after = model.npz_dict()
    assert all(np.array_equal(before[k], after[k]) for k in before) and tr.opt.t == 0
    for m, v in tr.opt.state.values():
        assert not bool(m.any()) and not bool(v.any())            # Adam's moments: still the zeros they started as
    assert int(model._overflow_flag(own.device).item()) == 0     # cleared with the error
    out = tr.step_from_tuples(_tuples(own, opp, act, z, visits), target="visits")   # the next good batch goes through
    assert tr.opt.t == 1 and np.isfinite(out["loss"])


@pytest.fixture(scope="module")
def self_play_tuples():
    """One small exploring self-play (the sizes of test_explore_gpu.py: 64 games, 24 playouts, explore_turns 8,
    random-init nets, the shipped rollout weights).  Returns (the policy the search used, the tuples)."""
    from iago_amd import engine, network, ops
    from tests.conftest import load_json
    torch.manual_seed(3)
    policy = network.SLPolicy().cuda().eval()
    value = network.Value().cuda().eval()
    g = load_json("simulate.json")
    m = engine.BatchedMCTS(64, policy, value, ops.RolloutWeights(g["shipped_w"], g["shipped_b"]), n_thr=15,
                           capacity=4096, seed=11, persistent=True)
    tup = engine.SelfPlayEngine(m).play(24, explore_turns=8).tuples()
    tup = {k: v.clone() for k, v in tup.items()}
    m.close()
    return policy, tup


def _trainer(policy):
    """A trainer on a fresh module with the policy's parameters (a module the search has used holds ctypes templates
    of its weights, which do not deep-copy)."""
    from iago_amd import network
    from iago_amd.train_rl import ReinforceTrainer
    model = network.SLPolicy()
    model.load_state_dict(policy.state_dict())
    return ReinforceTrainer(model, pool_dir=None, N=2, seed=1)


def test_the_trainer_steps_on_the_visit_counts_of_a_self_play(self_play_tuples):
    policy, tup = self_play_tuples
    assert tup["pi"].dtype == torch.int32 and tup["pi"].shape[1] == 64 and int(tup["pi"].min()) >= 0
    tr = _trainer(policy)
    outs = [tr.step_from_tuples(tup, target="visits") for _ in range(5)]
    for out in outs:
        assert set(out) >= {"loss", "kl", "n_tuples"} and np.isfinite(out["loss"])
        assert out["kl"] >= -1e-6 and out["n_tuples"] == tup["z"].numel()
    print("loss %s, kl %s" % ([round(o["loss"], 5) for o in outs], [round(o["kl"], 5) for o in outs]))
    assert outs[-1]["loss"] < outs[0]["loss"]
    assert tr.opt.t == 5


def test_target_move_is_the_step_as_it_was(self_play_tuples):
    policy, tup = self_play_tuples
    a, b = _trainer(policy), _trainer(policy)
    out_a = a.step_from_tuples(tup)
    out_b = b.step_from_tuples(tup, target="move")
    assert out_a == out_b and "kl" not in out_a
    for (k, pa), pb in zip(a.model1.named_parameters(), b.model1.parameters()):
        assert torch.equal(pa, pb), k
    with pytest.raises(ValueError, match="target"):
        a.step_from_tuples(tup, target="bogus")
    assert a.opt.t == 1


def test_a_float32_model_takes_the_autograd_update(self_play_tuples, monkeypatch):
    from iago_amd import network
    policy, tup = self_play_tuples
    tr = _trainer(policy)
    tr.model1.split3 = False
    called = []
    monkeypatch.setattr(network.SLPolicy, "visits_grads", lambda self, *a, **k: called.append(1))
    few = {k: v[:40] for k, v in tup.items()}                    # (40 rows run as 512: one batch shape for the library)
    out = tr.step_from_tuples(few, target="visits")
    assert not called and np.isfinite(out["loss"]) and out["kl"] >= -1e-6 and tr.opt.t == 1
