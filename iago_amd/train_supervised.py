"""Supervised trainers of the reference (train_policy.py:10-88, train_value.py:9-70)
on device-resident bitboard data sets: minibatches of 4096, Chainer's Adam with
the WeightDecay(5e-4) hook (train_rl.ChainerAdam), per-epoch test loss.

The reference's policy loss applies F.softmax_cross_entropy to the model's
OUTPUT, which is already a softmax (train_policy.py:59-60, network.py:46) -- the
same double softmax as in REINFORCE; it is reproduced here.  Data sets are
(own, opp, label) tensors with own = the side to move; the reference's
[x==1, x==2] planes of "white(2) to play" boards (load.py:41-47) are
encode_planes(own = the 2-stones, opp = the 1-stones).  Data preparation
(load.py) and the 8-fold augmentation are ops.augment8.

native=True computes every minibatch's loss and gradients with the split-f16
gradient kernels of the library (network.Value.value_grads,
network.SLPolicy.reinforce_grads) instead of autograd over the tensor
library's float32 convolutions; the optimiser step is the same.
"""
import torch
import torch.nn.functional as F

from . import _lib, network, ops
from .train_rl import ChainerAdam

MINIBATCH = 4096  # train_policy.py:43, train_value.py:33
DROPOUT_RATIO = 0.4  # network.py:95, F.dropout(h, 0.4) in training mode


def policy_loss(model, own, opp, actions):
    pred = model(ops.encode_planes(own, opp))                 # probabilities
    return F.cross_entropy(pred, actions.to(torch.int64)), pred  # softmax_cross_entropy(pred, y)


def value_loss(model, own, opp, results):
    pred = model(ops.encode_planes(own, opp))
    return F.mse_loss(pred, results.to(torch.float32)), pred   # mean_squared_error


class SupervisedTrainer(object):
    """kind = 'policy' (SLPolicy / RolloutPolicy, labels = actions) or 'value'
    (Value, labels = results).

    native=True: the minibatches' gradients come from the split-f16 kernels --
    Value + 'value' through Value.value_grads (iago_value_mse_grad), SLPolicy +
    'policy' through SLPolicy.reinforce_grads with every reward 1 (the
    supervised loss mean(softmax_cross_entropy(softmax(logits), y)) is the
    REINFORCE loss with r = 1).  Any other model, or a model set to
    `split_f16 = False` / `split3 = False`, raises ValueError.  The dropout of
    a native Value step draws its mask from the trainer's generator: per
    minibatch, right after that minibatch's slice of the epoch's permutation
    (torch.randperm(n, generator=self.gen) once per epoch),
    keep = torch.rand((m, 128), generator=self.gen) >= DROPOUT_RATIO.  A step
    whose forward left the f16 range raises IagoError and applies nothing."""

    def __init__(self, model, kind, seed=0, device="cuda", native=False):
        if kind not in ("policy", "value"):
            raise ValueError("kind must be 'policy' or 'value'")
        if native:
            if kind == "value" and isinstance(model, network.Value):
                if not model.split_f16:
                    raise ValueError("native=True: the Value net is set to split_f16 = False")
            elif kind == "policy" and isinstance(model, network.SLPolicy):
                if not model.split3:
                    raise ValueError("native=True: the SLPolicy net is set to split3 = False")
            else:
                raise ValueError("native=True trains Value ('value') or SLPolicy ('policy'), not %s ('%s')"
                                 % (type(model).__name__, kind))
        self.model, self.kind, self.native = model.to(device), kind, native
        self.opt = ChainerAdam(self.model)                     # optimizers.Adam() + WeightDecay(5e-4)
        self.gen = torch.Generator(device=device)
        self.gen.manual_seed(seed)
        self.loss_fn = policy_loss if kind == "policy" else value_loss

    def _native_step(self, own, opp, labels):
        """One minibatch through the gradient kernels, then Adam -- unless the forward saturated."""
        m = own.numel()
        if self.kind == "value":
            keep = torch.rand((m, 128), device=own.device, generator=self.gen) >= DROPOUT_RATIO
            loss = self.model.value_grads(own, opp, labels, keep=keep)
        else:
            ones = torch.ones(m, dtype=torch.float32, device=own.device)
            loss = self.model.reinforce_grads(own, opp, labels, ones)
        # the loss and the saturation word in ONE read-back, BEFORE Adam: the gradients of a clamped forward (or of a
        # label outside 0 .. 63) must not reach the parameters
        flag = self.model._overflow_flag(own.device)
        loss_v, bad = torch.stack([loss.to(torch.float64), flag[0].to(torch.float64)]).tolist()
        if bad:
            flag.zero_()
            raise _lib.IagoError(
                "supervised native step: %s; no update was applied.  Train with native=False (float32 autograd)"
                % ("a label lies outside 0 .. 63" if int(bad) & 2 else
                   "an activation of the forward left the f16 range of the split kernels (|a| > 65000) or is NaN"))
        self.opt.update()
        return loss_v

    def _step(self, own, opp, labels):
        """One minibatch update (the model in training mode): the loss as a Python float."""
        if self.native:
            return self._native_step(own, opp, labels)
        for p in self.model.parameters():
            p.grad = None
        loss, _ = self.loss_fn(self.model, own, opp, labels)
        loss.backward()
        self.opt.update()
        return float(loss.item())

    def step_rows(self, own, opp, labels):
        """One update on the given rows as ONE minibatch (rows sampled elsewhere: replay.ReplayWindow.sample's own, opp
        and `result` for a Value net) -- a minibatch of epoch() without the permutation; a native Value step draws its
        dropout mask from the trainer's generator as there.  Returns the loss."""
        self.model.train()
        return self._step(own, opp, labels)

    def epoch(self, own, opp, labels):
        """One shuffled sweep (train_policy.py:46-62); returns the mean minibatch loss."""
        n = own.numel()
        perm = torch.randperm(n, device=own.device, generator=self.gen)
        self.model.train()
        total, count = 0.0, 0
        for lo in range(0, n, MINIBATCH):
            idx = perm[lo:lo + MINIBATCH]
            total += self._step(own[idx], opp[idx], labels[idx])
            count += 1
        return total / max(count, 1)

    @torch.no_grad()
    def evaluate(self, own, opp, labels):
        """Test loss (and accuracy for policies), train_policy.py:63-68."""
        self.model.eval()
        n = own.numel()
        if n <= MINIBATCH:
            loss, pred = self.loss_fn(self.model, own, opp, labels)
            out = {"loss": float(loss.item())}
            if self.kind == "policy":
                out["accuracy"] = float((pred.argmax(dim=1) == labels.to(torch.int64)).float().mean())
            return out
        # a test set beyond one minibatch goes through in minibatches (the reference hands the whole set to the net at
        # once: activations of 128 x 64 floats per sample and layer, and a convolution shape MIOpen has not seen --
        # 22 s of solver search for 20,000 samples, measured); the means are the sample-weighted means of the pieces
        total = torch.zeros((), dtype=torch.float64, device=own.device)
        hits = torch.zeros((), dtype=torch.float64, device=own.device)
        for lo in range(0, n, MINIBATCH):
            sl = slice(lo, min(lo + MINIBATCH, n))
            loss, pred = self.loss_fn(self.model, own[sl], opp[sl], labels[sl])
            total += loss.to(torch.float64) * (sl.stop - sl.start)
            if self.kind == "policy":
                hits += (pred.argmax(dim=1) == labels[sl].to(torch.int64)).sum()
        out = {"loss": float((total / n).item())}
        if self.kind == "policy":
            out["accuracy"] = float((hits / n).item())
        return out
