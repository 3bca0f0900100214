"""The value targets without a GPU: the numpy restatement (tests/value_targets_ref.py) against the properties the rules
promise, the three entry points' place in their headers and bindings, the refusals that come before any device is
touched, the replay window's bookkeeping of the value column and the engine's refusals."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

from iago_amd import _lib, build, engine
from tests import value_targets_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q16 = 65536


def random_records(rs, T, B, kinds=(0, 1, 2, 3, 4, 5), q_max=1 << 30):
    valid = np.asarray(kinds, np.uint8)[rs.randint(len(kinds), size=(T, B))]
    q = rs.randint(-q_max, q_max + 1, size=(T, B), dtype=np.int64).astype(np.int32)
    score = rs.randint(-64, 65, size=(T, B)).astype(np.int8)
    z = rs.randint(-1, 2, size=B).astype(np.int8)
    mover = np.asarray([1 if t % 2 == 0 else 2 for t in range(T)], np.int8)
    return valid, q, score, z, mover


def sign_of(mover):
    return np.where(np.asarray(mover) == 1, 1, -1).reshape(-1, 1)


def test_the_worked_case():
    valid = np.ones((4, 1), np.uint8)
    q = np.array([[32768], [-16384], [49152], [-65536]], np.int32)
    out = ref.value_targets(valid, q, np.zeros((4, 1), np.int8), [1], [1, 2, 1, 2], 128, 0)
    assert out.dtype == np.int32 and out.reshape(-1).tolist() == [36864, -57344, 65536, -65536]


def test_lambda_one_without_mixing_is_the_result_from_the_movers_view():
    rs = np.random.RandomState(0)
    for T, B in ((1, 3), (9, 5), (60, 7)):
        valid, q, score, z, mover = random_records(rs, T, B)
        out = ref.value_targets(valid, q, score, z, mover, 256, 0)
        row = np.isin(valid, (1, 3, 4))
        want = Q16 * z.astype(np.int64).reshape(1, B) * sign_of(mover)
        assert np.array_equal(out, np.where(row, want, 0))


def test_one_step_bootstrapping_takes_the_next_rows_value():
    rs = np.random.RandomState(1)
    T, B = 12, 6
    valid, q, score, z, mover = random_records(rs, T, B, kinds=(1, 4), q_max=Q16)
    out = ref.value_targets(valid, q, score, z, mover, 0, 0)
    s = sign_of(mover)
    v1 = s * q.astype(np.int64)                                       # V_t in colour 1's frame (|q| <= 65536: no clip)
    nxt = np.concatenate([v1[1:], Q16 * z.astype(np.int64).reshape(1, B)])
    assert np.array_equal(out, s * nxt)
    # and with all of the row's own value mixed in, the row's own (clipped) q
    assert np.array_equal(ref.value_targets(valid, q, score, z, mover, 0, 256), q)


def test_rows_that_are_none_are_skipped_without_breaking_the_chain():
    # game 0: every turn searched; game 1: the same rows with a pass (0), a drawn row (2) and an opening row (5) between
    q0 = [30000, -20000, 10000, -5000]
    valid = np.array([[1, 1], [1, 0], [1, 2], [1, 5], [0, 1], [0, 1], [0, 1]], np.uint8)
    q = np.zeros((7, 2), np.int32)
    q[:4, 0] = q0
    q[[0, 4, 5, 6], 1] = q0
    q[1:4, 1] = 77777                                                  # (never read: no rows)
    mover = [1, 2, 1, 2, 2, 1, 2]                                      # game 1's rows 4 .. 6 move as game 0's 1 .. 3
    for lam, mix in ((128, 0), (243, 64), (0, 0), (256, 128)):
        out = ref.value_targets(valid, q, np.zeros((7, 2), np.int8), [1, 1], mover, lam, mix)
        assert out[:4, 0].tolist() == out[[0, 4, 5, 6], 1].tolist(), (lam, mix)
        assert out[1:4, 1].tolist() == [0, 0, 0] and out[4:, 0].tolist() == [0, 0, 0]


def test_a_solved_row_uses_the_sign_of_its_score():
    valid = np.array([[3], [3], [3]], np.uint8)
    score = np.array([[-12], [0], [64]], np.int8)
    q = np.full((3, 1), 12345, np.int32)                               # (not read on a solved row)
    out = ref.value_targets(valid, q, score, [0], [1, 2, 1], 0, 256)
    assert out.reshape(-1).tolist() == [-Q16, 0, Q16]
    # one step back from a solved row: its value from the other mover's view
    valid = np.array([[1], [3]], np.uint8)
    out = ref.value_targets(valid, np.zeros((2, 1), np.int32), np.array([[0], [-3]], np.int8), [1], [1, 2], 0, 0)
    assert out.reshape(-1).tolist() == [Q16, -Q16]                     # (colour 2 loses: +1 for colour 1; then Z for colour 2)


def test_q_is_clipped_in_the_targets_but_not_in_the_root_value():
    valid = np.ones((2, 1), np.uint8)
    q = np.array([[3 * Q16], [-(1 << 30)]], np.int32)
    out = ref.value_targets(valid, q, np.zeros((2, 1), np.int8), [0], [1, 2], 0, 256)
    assert out.reshape(-1).tolist() == [Q16, -Q16]
    got = ref.root_value_q16(np.array([-3.0, 2.5, -16383.0], np.float32))
    assert got.tolist() == [3 * Q16, -(5 * Q16) // 2, 16383 * Q16]


def test_root_value_rounds_to_even_and_saturates():
    half = 2.0 ** -17                                                   # half a Q16 step: exact in float32
    q = np.array([-0.5 * 2 ** -16, -1.5 * 2 ** -16, -2.5 * 2 ** -16, 0.5 * 2 ** -16, 1.5 * 2 ** -16, half * 3,
                  0.0, -0.0, 1.0, -1.0], np.float32)
    got, flags = ref.root_value_q16(q, with_flags=True)
    assert got.tolist() == [0, 2, 2, 0, -2, -2, 0, 0, -Q16, Q16] and flags == 0
    edge = np.float32(16384.0)                                          # 2^30 / 65536: the last value that is not saturated
    got, flags = ref.root_value_q16(np.array([-edge, edge], np.float32), with_flags=True)
    assert got.tolist() == [1 << 30, -(1 << 30)] and flags == 0
    above = np.nextafter(edge, np.float32(np.inf), dtype=np.float32)
    for bad in (above, np.float32(3e38), np.float32(np.inf)):
        got, flags = ref.root_value_q16(np.array([-bad, bad], np.float32), with_flags=True)
        assert got.tolist() == [1 << 30, -(1 << 30)] and flags == ref.SATURATED, bad
    got, flags = ref.root_value_q16(np.array([np.nan, 0.25], np.float32), with_flags=True)
    assert got.tolist() == [0, -16384] and flags == ref.NAN


def test_merge_values_sums_by_group():
    order = np.array([3, 0, 2, 1, 4], np.int32)
    group = np.array([0, 0, 1, 2, 2], np.int32)
    v = np.array([1 << 30, 5, -7, 1 << 30, 1 << 30], np.int32)
    got = ref.merge_values(order, group, v)
    assert got.dtype == np.int64 and got.tolist() == [1 << 31, -7, 5 + (1 << 30)]   # (a sum that leaves int32)


# ---- the entry points: headers, bindings, refusals ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def so():
    return build.build()


def declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    return set(re.findall(r"IAGO_API[^;(]*?\b(iago_\w+)\s*\(", text))


def test_the_entry_points_are_declared_listed_and_exported(so):
    core = declared("iago_hip.h")
    exported = set(re.findall(r" T (iago_\w+)", subprocess.check_output(["nm", "-D", "--defined-only", so]).decode()))
    L = _lib.lib()
    for name, header, names in (("iago_mcts_root_value", "iago_hip_serving.h", _lib.SERVING_SYMBOLS),
                                ("iago_value_targets", "iago_hip_training.h", _lib.TRAINING_SYMBOLS),
                                ("iago_replay_merge_values", "iago_hip_training.h", _lib.TRAINING_SYMBOLS)):
        assert name in declared(header) and name in names and name not in core and name not in _lib.SYMBOLS, name
        assert name in exported and hasattr(L, name), name
    assert L.iago_abi_version() == _lib.ABI_VERSION == 13


FAKE = 0x1000   # a pointer that is never dereferenced: the checks come first


def _refused(name, rc):
    assert rc == _lib.IAGO_ERR_INVALID
    msg = _lib.lib().iago_last_error()
    assert name.encode() in msg, msg
    return msg


def _tree(n_games=4, capacity=16, **kw):
    t = _lib.MctsTree()
    t.n_games, t.capacity, t.has_v = n_games, capacity, 0
    t.nodes, t.n_nodes, t.root, t.overflow = FAKE, FAKE, FAKE, FAKE
    for k, v in kw.items():
        setattr(t, k, v)
    return t


def test_root_value_refuses_before_any_launch(so):
    L, name = _lib.lib(), "iago_mcts_root_value"
    _refused(name, L.iago_mcts_root_value(None, FAKE, FAKE, FAKE, None, None))
    for bad in (dict(nodes=None), dict(root=None), dict(n_nodes=None), dict(capacity=0), dict(n_games=-1)):
        _refused(name, L.iago_mcts_root_value(C.byref(_tree(**bad)), FAKE, FAKE, FAKE, None, None))
    assert b"n_games" in _refused(name, L.iago_mcts_root_value(C.byref(_tree(n_games=0)), FAKE, FAKE, FAKE, None, None))
    for args in ((None, FAKE, FAKE), (FAKE, None, FAKE), (FAKE, FAKE, None)):
        assert b"null" in _refused(name, L.iago_mcts_root_value(C.byref(_tree()), *args, None, None))


def _target_args(**kw):
    a = _lib.ValueTargetsArgs()
    a.valid = a.q = a.score = a.z = a.mover = a.out = FAKE
    a.n_turns, a.n_games, a.lam_256, a.mix_256 = 4, 8, 256, 0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_value_targets_refuses_before_any_launch(so):
    L, name = _lib.lib(), "iago_value_targets"
    _refused(name, L.iago_value_targets(None, None))
    for field in ("valid", "q", "score", "z", "mover", "out"):
        assert b"null" in _refused(name, L.iago_value_targets(C.byref(_target_args(**{field: None})), None))
    for bad in (dict(n_turns=0), dict(n_turns=-2), dict(n_games=0), dict(n_games=-1), dict(n_turns=1 << 20, n_games=1 << 20)):
        _refused(name, L.iago_value_targets(C.byref(_target_args(**bad)), None))
    for bad in (dict(lam_256=-1), dict(lam_256=257), dict(mix_256=-1), dict(mix_256=257), dict(lam_256=1 << 20)):
        assert b"[0, 256]" in _refused(name, L.iago_value_targets(C.byref(_target_args(**bad)), None))


def _merge_args(**kw):
    a = _lib.ReplayMergeValuesArgs()
    a.order = a.group = a.first = a.mult = a.v = a.v_sum = FAKE
    a.count, a.n_unique = 8, 3
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_merge_values_refuses_before_any_launch(so):
    L, name = _lib.lib(), "iago_replay_merge_values"
    _refused(name, L.iago_replay_merge_values(None, None))
    for field in ("order", "group", "first", "mult", "v", "v_sum"):
        assert b"null" in _refused(name, L.iago_replay_merge_values(C.byref(_merge_args(**{field: None})), None))
    for bad in (dict(count=0), dict(count=-1), dict(count=1 << 31), dict(n_unique=0), dict(n_unique=9)):
        _refused(name, L.iago_replay_merge_values(C.byref(_merge_args(**bad)), None))


def test_the_wrappers_refuse_bad_rates_before_any_device():
    from iago_amd import ops
    t = torch.zeros((2, 2), dtype=torch.uint8)
    for lam, mix in ((-1, 0), (257, 0), (0, 300), (1.5, 0), (True, 0), (None, 0)):
        with pytest.raises(ValueError, match="256"):
            ops.value_targets(t, t, t, t, [1, 2], lam, mix)


# ---- the window's value column, the rules record and the engine's refusals, on the CPU -----------------------------------

def _rows(lo, n, with_v=True):
    own = torch.arange(lo, lo + n)
    rows = dict(own=own, opp=own << 20, pi=torch.ones((n, 64), dtype=torch.int32) * own.reshape(n, 1).to(torch.int32),
                move=(own % 60).to(torch.int8), z=(own % 3 - 1).to(torch.int8))
    if with_v:
        rows["v"] = (1000 * own - 7).to(torch.int32)
    return rows


def test_a_window_with_value_targets_needs_the_column_and_wraps_it_with_the_others():
    from iago_amd.replay import ReplayWindow
    w = ReplayWindow(capacity=8, device="cpu", value_targets=True)
    assert w.value_targets and w.cols["v"].dtype == torch.int32 and tuple(w.cols["v"].shape) == (8,)
    with pytest.raises(ValueError, match="v"):
        w.add(_rows(1, 4, with_v=False))
    assert w.total == 0                                               # (a refused batch adds nothing)
    assert w.add(_rows(1, 6)) == 6 and w.add(_rows(7, 5)) == 5        # rows 1 .. 11: row r of all lives in slot r % 8
    assert w.total == 11 and w.count == 8
    own = w.cols["own"].tolist()
    assert own == [9, 10, 11, 4, 5, 6, 7, 8]
    assert w.cols["v"].tolist() == [1000 * x - 7 for x in own]
    assert w.cols["move"].tolist() == [x % 60 for x in own] and w.cols["pi"][:, 5].tolist() == own
    assert w.add(_rows(100, 20)) == 20                                # (of a batch larger than the window the last 8 stay)
    assert sorted(w.cols["v"].tolist()) == [1000 * x - 7 for x in range(112, 120)]


def test_a_window_without_value_targets_is_the_window_of_before():
    from iago_amd.replay import ReplayWindow
    w = ReplayWindow(capacity=8, device="cpu")
    assert not w.value_targets and sorted(w.cols) == ["move", "opp", "own", "pi", "z"]
    assert w.add(_rows(1, 4, with_v=False)) == 4 and w.add(_rows(5, 2)) == 2   # (other keys are ignored, v among them)
    assert sorted(w.cols) == ["move", "opp", "own", "pi", "z"]


def test_play_rules_default_and_validation():
    assert engine.NO_RULES.root_values is False and engine.PlayRules(None, 0, None).root_values is False
    assert engine._play_rules(16).root_values is False and engine._play_rules(16) == engine.NO_RULES
    r = engine._play_rules(16, solve_empties=6, explore_turns=2, root_values=True)
    assert r.root_values is True and r[:7] == engine._play_rules(16, solve_empties=6, explore_turns=2)[:7]
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="root_values"):
            engine._play_rules(16, root_values=bad)


def test_root_values_need_the_negamax_backup():
    m = types.SimpleNamespace(backup="reference", persistent=True, rollout_hook=None)
    with pytest.raises(ValueError, match="negamax"):
        engine.BatchedMCTS.root_value(m)
    with pytest.raises(ValueError, match="negamax"):
        engine.BatchedMCTS.root_value(types.SimpleNamespace())       # (an engine of before: the reference's rule)
    with pytest.raises(ValueError, match="negamax"):                 # refused where a round begins, before anything is reset
        engine.BatchedMCTS._backup_check(m, engine._play_rules(16, root_values=True))
    engine.BatchedMCTS._backup_check(m, engine._play_rules(16))
    engine.BatchedMCTS._backup_check(types.SimpleNamespace(backup="negamax", persistent=True, rollout_hook=None),
                                     engine._play_rules(16, root_values=True))


def test_value_targets_of_a_result_without_the_record_are_refused():
    res = engine.SelfPlayResult()
    assert res.q is None and res.q_visits is None
    with pytest.raises(ValueError, match="root_values"):
        res.value_targets(128, 64)
