"""include/iago_hip_training.h: its symbols are the bindings' TRAINING_SYMBOLS and the library exports them, and
iago_value_mse_grad refuses bad arguments before it touches a device (no GPU here)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from iago_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def so():
    return build.build()


def header_symbols(name):
    text = open(os.path.join(ROOT, "include", name)).read()
    return sorted(set(re.findall(r"IAGO_API[^;(]*?\b(iago_\w+)\s*\(", text)))


def test_training_header_matches_its_symbol_list(so):
    assert header_symbols("iago_hip_training.h") == sorted(_lib.TRAINING_SYMBOLS)
    others = _lib.SYMBOLS + _lib.LAYER_SYMBOLS + _lib.EXPERIMENTAL_SYMBOLS + _lib.SERVING_SYMBOLS
    assert not set(_lib.TRAINING_SYMBOLS) & set(others)
    out = subprocess.check_output(["nm", "-D", "--defined-only", so]).decode()
    exported = set(re.findall(r" T (iago_\w+)", out))
    assert set(_lib.TRAINING_SYMBOLS) <= exported
    L = _lib.lib()
    for name in _lib.TRAINING_SYMBOLS:
        assert hasattr(L, name), name
    assert L.iago_abi_version() == 13


def test_workspace_bytes(so):
    L = _lib.lib()
    assert L.iago_value_grad_workspace_bytes(-1) == -1
    sizes = [L.iago_value_grad_workspace_bytes(n) for n in (0, 1, 256, 4096, 10000)]
    assert all(a < b for a, b in zip(sizes, sizes[1:]))
    assert sizes[-1] > 2 ** 31                                   # (a 64-bit result)
    for n in (1, 4096):                                          # the trunk's scratch, then the head's
        assert L.iago_value_grad_workspace_bytes(n) > L.iago_policy_grad_workspace_bytes(n)


def _args(n=4, n_mean=4, scale=1.0 / 0.6, ws_bytes=None, ws_addr=1 << 20):
    """Arguments with every pointer set to a fake (never dereferenced: the checks come first)."""
    L = _lib.lib()
    a = _lib.ValueGradArgs()
    fake = 0x1000
    for name, typ in _lib.ValueGradArgs._fields_:
        if typ is C.c_void_p:
            setattr(a, name, fake)
        elif name in ("w_hi", "w_lo", "wt_hi", "wt_lo", "bias", "g_w", "g_b"):
            arr = getattr(a, name)
            for k in range(7):
                arr[k] = fake
    a.keep = None
    a.pred = a.h9 = a.overflow = None
    a.n, a.n_mean, a.dropout_scale = n, n_mean, scale
    a.workspace = ws_addr
    a.workspace_bytes = L.iago_value_grad_workspace_bytes(max(n, 0)) if ws_bytes is None else ws_bytes
    return a


def _refused(a):
    L = _lib.lib()
    rc = L.iago_value_mse_grad(C.byref(a) if a is not None else None, None)
    assert rc == -1                                              # IAGO_ERR_INVALID
    msg = L.iago_last_error()
    assert b"iago_value_mse_grad" in msg
    return msg


def test_bad_arguments_are_refused_before_any_launch(so):
    L = _lib.lib()
    _refused(None)
    _refused(_args(n=0))
    _refused(_args(n=-3))
    _refused(_args(n_mean=0))
    _refused(_args(n_mean=-1))
    for field in ("own", "opp", "result", "w1", "b1", "w9", "b9", "w10", "w11", "g_w1", "g_b1", "g_w9", "g_b9",
                  "g_w10", "g_w11", "loss", "workspace"):
        a = _args()
        setattr(a, field, None)
        assert b"null" in _refused(a), field
    for field in ("w_hi", "wt_lo", "bias", "g_w", "g_b"):
        a = _args()
        getattr(a, field)[3] = None
        assert b"null" in _refused(a), field
    a = _args()
    a.workspace_bytes -= 1
    assert b"workspace" in _refused(a)
    assert b"workspace" in _refused(_args(ws_addr=(1 << 20) + 128))
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert b"dropout_scale" in _refused(_args(scale=bad))
    # (the checks need no device: a host without one gets the same answers)
    assert L.iago_value_grad_workspace_bytes(8) > 0
