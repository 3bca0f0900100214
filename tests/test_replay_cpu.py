"""The replay window without a GPU (iago_replay_sample, replay.ReplayWindow): the entry point's place in the headers
and bindings, its refusals before any device is touched, the numpy reference of its symmetries (tests/replay_ref.py)
against the oracle's augmentation and the oracle's rules, and the ring's bookkeeping on the CPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from iago_amd import _lib, build
from oracle import augment_np
from oracle import oracle as orc
from tests import replay_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def so():
    return build.build()


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    return set(re.findall(r"IAGO_API[^;(]*?\b(iago_\w+)\s*\(", text))


def test_the_entry_point_is_in_the_training_header_only(so):
    assert "iago_replay_sample" in _declared("iago_hip_training.h")
    assert "iago_replay_sample" not in _declared("iago_hip.h")
    assert "iago_replay_sample" in _lib.TRAINING_SYMBOLS
    out = subprocess.check_output(["nm", "-D", "--defined-only", so]).decode()
    assert "iago_replay_sample" in set(re.findall(r" T (iago_\w+)", out))
    L = _lib.lib()
    assert hasattr(L, "iago_replay_sample") and L.iago_abi_version() == 13


OPTIONAL = ("slot_in", "sym_in", "result_out", "slot_out", "sym_out", "flags")


def _args(capacity=8, count=3, n=5, given=False):
    """Arguments with every required pointer set to a fake (never dereferenced: the checks come first)."""
    a = _lib.ReplaySampleArgs()
    for name, typ in _lib.ReplaySampleArgs._fields_:
        if typ is C.c_void_p and (name not in OPTIONAL or (given and name in ("slot_in", "sym_in"))):
            setattr(a, name, 0x1000)
    a.capacity, a.count, a.n, a.seed, a.step = capacity, count, n, 7, 1
    return a


def _refused(a):
    L = _lib.lib()
    rc = L.iago_replay_sample(C.byref(a) if a is not None else None, None)
    assert rc == -1                                              # IAGO_ERR_INVALID
    msg = L.iago_last_error()
    assert b"iago_replay_sample" in msg
    return msg


def test_bad_arguments_are_refused_before_any_launch(so):
    _refused(None)
    for field in ("own", "opp", "pi", "move", "z", "own_out", "opp_out", "pi_out", "move_out", "z_out"):
        for given in (False, True):
            a = _args(given=given)
            setattr(a, field, None)
            assert b"null" in _refused(a), field
    for n in (0, -1):
        assert b"n must" in _refused(_args(n=n))
    for count in (0, -2):
        assert b"count" in _refused(_args(count=count))
    assert b"count" in _refused(_args(capacity=8, count=9))
    assert b"count" in _refused(_args(capacity=2 ** 31, count=1))
    for only in ("slot_in", "sym_in"):
        a = _args()
        setattr(a, only, 0x1000)
        assert b"both or neither" in _refused(a), only


@pytest.fixture(scope="module")
def positions():
    """64 positions of random legal play, 1 .. 60 plies in: (state as the oracle's 8 x 8 array, the colour to move)."""
    rs = np.random.RandomState(5)
    out = []
    while len(out) < 64:
        s, colour = orc.initial_state(), 1
        for _ in range(rs.randint(1, 61)):
            acts = orc.legal_actions(s, colour)
            if not acts:
                colour = 3 - colour
                acts = orc.legal_actions(s, colour)
                if not acts:
                    break
            orc.place_stone(s, acts[rs.randint(len(acts))], colour)
            colour = 3 - colour
        if orc.legal_actions(s, colour):
            out.append((s.copy(), colour))
    return out


def test_cell_maps_are_the_oracles_augmentation(positions):
    rs = np.random.RandomState(6)
    for k in range(8):
        m = replay_ref.cell_map(k)
        assert sorted(m) == list(range(64))
    for s, colour in positions:
        p1, p2 = orc.state_to_bits(s)
        own, opp = (p1, p2) if colour == 1 else (p2, p1)
        move = int(rs.randint(64))
        pi = rs.randint(0, 50, size=64)
        S, A = augment_np.augment8(s[None], np.array([move]))
        # the visit row as a board of its own: the augmentation moves its cells as it moves the stones
        P, _ = augment_np.augment8(pi.reshape(1, 8, 8), np.array([move]))
        for k in range(8):
            o, p, pk, mk = replay_ref.apply(own, opp, pi, move, k)
            q1, q2 = (o, p) if colour == 1 else (p, o)
            assert np.array_equal(orc.bits_to_state(q1, q2).reshape(8, 8), S[k, 0]), k
            assert mk == int(A[k, 0]) == replay_ref.cell_map(k)[move]
            assert np.array_equal(pk.reshape(8, 8), P[k, 0]), k
            assert replay_ref.apply(own, opp, pi, -1, k)[3] == -1


def test_the_transformed_boards_legal_moves_are_the_transformed_legal_moves(positions):
    for s, colour in positions:
        legal = orc.legal_actions(s, colour)
        p1, p2 = orc.state_to_bits(s)
        for k in range(8):
            m = replay_ref.cell_map(k)
            q1, q2, _, _ = replay_ref.apply(p1, p2, np.zeros(64, np.int32), -1, k)
            got = orc.legal_actions(orc.bits_to_state(q1, q2).reshape(8, 8), colour)
            assert sorted(got) == sorted(m[a] for a in legal), k


def test_draws_stay_in_range_and_follow_the_key():
    slots, syms = set(), set()
    for j in range(200):
        slot, sym = replay_ref.draw(3, 0, j, 5)
        assert 0 <= slot < 5 and 0 <= sym < 8
        slots.add(slot)
        syms.add(sym)
    # (a uniform draw misses one of 8 values in 200 tries with probability 8 (7/8)^200 < 1e-10)
    assert slots == set(range(5)) and syms == set(range(8))
    assert replay_ref.draw(3, 0, 0, 1)[0] == 0
    a = [replay_ref.draw(3, 0, j, 1000) for j in range(8)]
    assert a != [replay_ref.draw(3, 1, j, 1000) for j in range(8)]
    assert a != [replay_ref.draw(4, 0, j, 1000) for j in range(8)]
    assert a != [replay_ref.draw(3 ^ (1 << 40), 0, j, 1000) for j in range(8)]


def _rows(lo, hi):
    """Rows lo .. hi-1 of a stream in which row r carries r in every column."""
    r = torch.arange(lo, hi)
    return dict(own=r.to(torch.int64) * 3, opp=r.to(torch.int64) * 5 + 1, pi=(r.reshape(-1, 1) * 64 +
                torch.arange(64)).to(torch.int32), move=(r % 64).to(torch.int8), z=(r % 3 - 1).to(torch.int8),
                colour=torch.ones(hi - lo, dtype=torch.int8))     # (a key add() ignores)


def _holds(w, slot, r):
    want = _rows(r, r + 1)
    return all(torch.equal(w.cols[k][slot], want[k][0]) for k in ("own", "opp", "pi", "move", "z"))


def test_the_ring_keeps_row_r_in_slot_r_mod_capacity():
    from iago_amd.replay import ReplayWindow
    w = ReplayWindow(capacity=5, device="cpu")
    assert (w.count, w.total) == (0, 0)
    with pytest.raises(ValueError, match="empty"):
        w.sample(4)
    assert w.step == 0
    w.add(_rows(0, 3))
    assert (w.count, w.total) == (3, 3)
    w.add(_rows(3, 7))
    assert (w.count, w.total) == (5, 7)
    assert _holds(w, 0, 5) and _holds(w, 1, 6) and _holds(w, 2, 2) and _holds(w, 3, 3) and _holds(w, 4, 4)
    assert w.cols["pi"].dtype == torch.int32 and w.cols["own"].dtype == torch.int64


def test_a_batch_larger_than_the_window_keeps_its_last_rows():
    from iago_amd.replay import ReplayWindow
    w = ReplayWindow(capacity=5, device="cpu")
    w.add(_rows(0, 12))
    assert (w.count, w.total) == (5, 12)
    for r in range(7, 12):
        assert _holds(w, r % 5, r)
    w.add(_rows(12, 14))
    assert (w.count, w.total) == (5, 14) and _holds(w, 12 % 5, 12) and _holds(w, 13 % 5, 13) and _holds(w, 1, 11)
    with pytest.raises(ValueError):
        ReplayWindow(capacity=0, device="cpu")
    with pytest.raises(ValueError, match="shape"):
        w.add(dict(_rows(0, 2), pi=torch.zeros(2, 63, dtype=torch.int32)))
