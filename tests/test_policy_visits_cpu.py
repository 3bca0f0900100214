"""Training SLPolicy on the search's visit counts, the parts that need no GPU: iago_policy_visits_grad is declared in
include/iago_hip_training.h, bound and exported, and refuses bad arguments before it touches a device; the loss
formula train_rl.visits_loss_from_logits against a numpy restatement written here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from iago_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "iago_policy_visits_grad"
ARRAYS = ("w_hi", "w_lo", "wt_hi", "wt_lo", "bias", "g_w", "g_b")


@pytest.fixture(scope="module")
def so():
    return build.build()


def test_the_entry_point_is_declared_bound_and_exported(so):
    text = open(os.path.join(ROOT, "include", "iago_hip_training.h")).read()
    assert re.search(r"IAGO_API\s+int\s+%s\s*\(\s*const\s+%s_args\s*\*" % (NAME, NAME), text)
    assert NAME in _lib.TRAINING_SYMBOLS
    assert NAME not in open(os.path.join(ROOT, "include", "iago_hip.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", so]).decode()
    assert re.search(r" T %s\b" % NAME, out)
    L = _lib.lib()
    assert hasattr(L, NAME) and L.iago_abi_version() == 13
    # iago_policy_grad_args with action / reward replaced by visits / weight: the same layout
    mine, theirs = _lib.PolicyVisitsGradArgs, _lib.PolicyGradArgs
    assert C.sizeof(mine) == C.sizeof(theirs)
    swapped = {"action": "visits", "reward": "weight"}
    assert [(swapped.get(f, f), t) for f, t in theirs._fields_] == list(mine._fields_)
    for f, _ in mine._fields_:
        assert getattr(mine, f).offset == getattr(theirs, {v: k for k, v in swapped.items()}.get(f, f)).offset


def _args(n=4, n_mean=4, ws_bytes=None, ws_addr=1 << 20):
    """Arguments with every pointer set to a fake (never dereferenced: the checks come first)."""
    L = _lib.lib()
    a = _lib.PolicyVisitsGradArgs()
    fake = 0x1000
    for name, typ in _lib.PolicyVisitsGradArgs._fields_:
        if typ is C.c_void_p:
            setattr(a, name, fake)
        elif name in ARRAYS:
            arr = getattr(a, name)
            for k in range(7):
                arr[k] = fake
    a.weight = a.probs = a.overflow = None                       # the optional ones
    a.n, a.n_mean = n, n_mean
    a.workspace = ws_addr
    a.workspace_bytes = L.iago_policy_grad_workspace_bytes(max(n, 0)) if ws_bytes is None else ws_bytes
    return a


def _refused(a):
    L = _lib.lib()
    rc = L.iago_policy_visits_grad(C.byref(a) if a is not None else None, None)
    assert rc == -1                                              # IAGO_ERR_INVALID
    msg = L.iago_last_error()
    assert NAME.encode() in msg
    return msg


def test_bad_arguments_are_refused_before_any_launch(so):
    _refused(None)
    _refused(_args(n=0))
    _refused(_args(n=-3))
    _refused(_args(n_mean=0))
    _refused(_args(n_mean=-1))
    for field in ("own", "opp", "visits", "w1", "b1", "w9", "b10", "g_w1", "g_b1", "g_w9", "g_b10", "loss",
                  "workspace"):
        a = _args()
        setattr(a, field, None)
        assert b"null" in _refused(a), field
    for field in ARRAYS:
        for k in (0, 3, 6):
            a = _args()
            getattr(a, field)[k] = None
            assert b"null" in _refused(a), (field, k)
    a = _args()
    a.workspace_bytes -= 1
    assert b"workspace" in _refused(a)
    assert b"workspace" in _refused(_args(ws_addr=(1 << 20) + 128))


def _case():
    """Logits (37, 64), visit rows with a one-hot row, an all-zero row, zeros among non-zeros, and weights."""
    rs = np.random.RandomState(5)
    logits = rs.randn(37, 64) * 3.0
    visits = rs.randint(0, 41, size=(37, 64)).astype(np.int32)
    visits[rs.rand(37, 64) < 0.6] = 0                            # zeros among non-zeros, as illegal cells are
    visits[0] = 0
    visits[0, 19] = 24                                           # one-hot
    visits[5] = 0                                                # no visits at all
    visits[9, :32] = 0
    assert (visits[9] > 0).any() and (visits.sum(axis=1) > 0).sum() == 36
    weight = rs.uniform(0.25, 2.0, size=37)
    return logits, visits, weight


def _numpy_loss(logits, visits, weight, n_mean):
    """The formula of include/iago_hip_training.h, row by row in float64.  Returns (loss, dlogits)."""
    loss, dl = 0.0, np.zeros_like(logits)
    for b in range(logits.shape[0]):
        m = logits[b].max()
        s = np.exp(logits[b] - m).sum()
        p = np.exp(logits[b] - m) / s
        N = int(visits[b].sum())
        if N == 0:
            continue
        t = visits[b] / float(N)
        hit = visits[b] > 0
        loss += weight[b] * -(t[hit] * ((logits[b][hit] - m) - np.log(s))).sum() / n_mean
        dl[b] = weight[b] / n_mean * (p - t)
    return loss, dl


@pytest.mark.parametrize("weighted,n_mean", [(True, None), (True, 50), (False, None)])
def test_the_loss_formula_against_numpy(weighted, n_mean):
    from iago_amd.train_rl import visits_loss_from_logits
    logits, visits, weight = _case()
    x = torch.tensor(logits, dtype=torch.float64, requires_grad=True)
    w = torch.tensor(weight, dtype=torch.float64) if weighted else None
    loss = visits_loss_from_logits(x, torch.from_numpy(visits), w, n_mean=n_mean)
    assert loss.dtype == torch.float64
    loss.backward()
    want, want_dl = _numpy_loss(logits, visits, weight if weighted else np.ones(37), 37 if n_mean is None else n_mean)
    assert abs(loss.item() - want) <= 1e-12
    assert float(np.abs(x.grad.numpy() - want_dl).max()) <= 1e-12
    assert bool((x.grad[5] == 0).all())                          # the all-zero row: exactly nothing


def test_a_cell_whose_probability_underflows_keeps_the_loss_finite():
    from iago_amd.train_rl import visits_loss_from_logits
    logits = torch.zeros(2, 64, dtype=torch.float32)
    logits[0, 3] = -200.0                                        # exp(-200) is 0 in float32: log(p) would be -inf
    logits[1, 7] = -float("inf")                                 # a masked cell without visits drops out
    visits = torch.zeros(2, 64, dtype=torch.int32)
    visits[0, 3], visits[0, 4], visits[1, 8] = 5, 5, 3
    x = logits.clone().requires_grad_(True)
    loss = visits_loss_from_logits(x, visits)
    loss.backward()
    assert np.isfinite(loss.item()) and loss.item() > 50.0 and bool(torch.isfinite(x.grad).all())


def test_one_hot_rows_weighted_by_r_are_the_weighted_cross_entropy():
    from iago_amd.train_rl import visits_loss_from_logits
    rs = np.random.RandomState(8)
    logits = torch.tensor(rs.randn(37, 64) * 2.0, dtype=torch.float64)
    a = torch.tensor(rs.randint(0, 64, size=37), dtype=torch.int64)
    r = torch.tensor(rs.choice([-1.0, 0.0, 1.0], size=37), dtype=torch.float64)
    visits = torch.zeros(37, 64, dtype=torch.int32)
    visits[torch.arange(37), a] = torch.tensor(rs.randint(1, 41, size=37), dtype=torch.int32)
    x1 = logits.clone().requires_grad_(True)
    visits_loss_from_logits(x1, visits, r).backward()
    x2 = logits.clone().requires_grad_(True)
    torch.mean(F.cross_entropy(x2, a, reduction="none") * r).backward()
    assert float((x1.grad - x2.grad).abs().max()) <= 1e-12


def test_step_from_tuples_refuses_an_unknown_target_before_it_gathers_anything():
    from iago_amd.train_rl import ReinforceTrainer
    tr = ReinforceTrainer.__new__(ReinforceTrainer)              # (no model, no device: the check comes first)
    with pytest.raises(ValueError, match="target"):
        tr.step_from_tuples({}, target="bogus")
