"""The host side of playing the endgame of whole games with the exact solver: the two entry points in the header, the
bindings and the library, their refusals before any device work, SelfPlayEngine's check of solve_empties, and the host
reference of iago_play_endgame (tests/endgame_play_ref.py) against the C reference solver.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import oracle as orc

from . import endgame_play_ref as play_ref
from . import endgame_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("iago_play_endgame", "iago_mcts_search_park")


def _lib():
    from iago_amd import _lib
    return _lib


def _error():
    return _lib().lib().iago_last_error().decode()


# ---------------------------------------------------------------- header, bindings, library
def test_entry_points_in_header_bindings_and_library():
    L = _lib()
    with open(os.path.join(ROOT, "include", "iago_hip_serving.h")) as f:
        header = f.read()
    for name in ENTRY_POINTS:
        assert re.search(r"IAGO_API int %s\(" % name, header), name
        assert name in L.SERVING_SYMBOLS
        assert getattr(L.lib(), name) is not None
    assert "iago_search_park_args" in header and "iago_play_endgame_args" in header
    assert L.lib().iago_abi_version() == 13 == L.ABI_VERSION


def test_struct_mirrors_have_the_header_sizes():
    L = _lib()
    # iago_play_endgame_args: 6 pointers, n, stride, 4 int32, 7 pointers, 4 reserved words
    assert C.sizeof(L.PlayEndgameArgs) == 6 * 8 + 2 * 8 + 4 * 4 + 7 * 8 + 4 * 8
    # iago_search_park_args: 2 int32, 4 pointers, 4 reserved words
    assert C.sizeof(L.SearchParkArgs) == 2 * 4 + 4 * 8 + 4 * 8


# ---------------------------------------------------------------- refusals (nothing is launched: the pointers are host memory)
def _play_args(n=4):
    L = _lib()
    keep = [np.zeros(128 * max(n, 1), np.int64) for _ in range(13)]
    a = L.PlayEndgameArgs()
    for name, buf in zip(("own", "opp", "turn", "stones", "pass_flg", "parked", "rec_own", "rec_opp", "rec_valid",
                          "rec_move", "rec_score", "finished", "ctl"), keep):
        setattr(a, name, buf.ctypes.data)
    a.n, a.stride, a.max_turns, a.max_empties, a.time_limit_ms = n, n, 128, 10, 1000
    return a, keep


@pytest.mark.parametrize("field,value", [
    ("n", -1), ("stride", 3), ("reserved0", 1), ("reserved", 1), ("max_turns", 0), ("max_turns", 129),
    ("max_empties", -1), ("max_empties", 21), ("time_limit_ms", 0), ("time_limit_ms", 600001), ("ctl", None),
    ("finished", None), ("rec_score", None)])
def test_play_endgame_refusals(field, value):
    L = _lib()
    a, keep = _play_args()
    if field == "reserved":
        a.reserved[2] = value
    else:
        setattr(a, field, value)
    assert L.lib().iago_play_endgame(C.byref(a), None) == -1
    assert _error().startswith("iago_play_endgame:")


def test_play_endgame_null_args():
    assert _lib().lib().iago_play_endgame(None, None) == -1
    assert _error() == "iago_play_endgame: null args"


def _park_args(codes=(1, 1, 1, 1)):
    L = _lib()
    active = np.array(codes, np.uint8)
    out = [np.zeros(16, np.int32) for _ in range(3)]
    tree = L.MctsTree()
    tree.n_games = len(codes)
    a = L.MctsSearchArgs()
    a.tree, a.active, a.max_turns = C.addressof(tree), active.ctypes.data, 128
    k = L.SearchParkArgs()
    k.park_empties = 8
    k.parked, k.stones, k.pass_flg = (b.ctypes.data for b in out)
    return a, k, (active, out, tree)


def test_search_park_refusals():
    L = _lib()
    f = L.lib().iago_mcts_search_park

    def refused(a, k, what):
        assert f(C.byref(a) if a is not None else None, C.byref(k) if k is not None else None, None) == -1
        assert _error().startswith("iago_mcts_search_park:") and what in _error(), _error()

    a, k, keep = _park_args()
    refused(None, k, "null args")
    refused(a, None, "null args")
    for bad in (-1, 21):
        a, k, keep = _park_args()
        k.park_empties = bad
        refused(a, k, "park_empties")
    a, k, keep = _park_args()
    k.reserved0 = 1
    refused(a, k, "reserved")
    a, k, keep = _park_args()
    k.reserved[3] = 7
    refused(a, k, "reserved")
    a, k, keep = _park_args()
    k.parked = None
    refused(a, k, "parked")
    a, k, keep = _park_args()
    a.max_turns = 0
    refused(a, k, "max_turns")
    for codes in ((1, 2, 1, 1), (3, 3, 3, 3), (0, 1, 1, 3)):
        a, k, keep = _park_args(codes)
        refused(a, k, "match codes")


# ---------------------------------------------------------------- the engine's check of solve_empties
class _StubMcts(object):
    """What SelfPlayEngine reads before its first device call; anything else is a failure of the test."""
    n_games = 4

    def __getattr__(self, name):
        raise AssertionError("solve_empties must be checked before the engine is touched (read %r)" % name)


@pytest.mark.parametrize("bad", [True, False, -1, 21, 8.0, "8", np.float32(3)])
def test_solve_empties_is_validated_before_the_device(bad):
    from iago_amd.engine import SelfPlayEngine
    e = SelfPlayEngine(_StubMcts())
    for call in (lambda: e.play(100, solve_empties=bad), lambda: e.play_stream(100, 8, solve_empties=bad),
                 lambda: e.play_match(100, solve_empties=bad)):
        with pytest.raises(ValueError, match="solve_empties"):
            call()


def test_solve_empties_accepts_the_range():
    from iago_amd.engine import _solve_empties_arg
    assert _solve_empties_arg(None) is None
    assert [_solve_empties_arg(k) for k in (0, 8, 20, np.int64(7))] == [0, 8, 20, 7]


# ---------------------------------------------------------------- the host reference
def _golden_late(golden_rules, lo, hi):
    own, opp = ref.golden_positions(golden_rules["trace"], lo, hi)
    return [(int(a), int(b)) for a, b in zip(own, opp)]


def test_play_ref_against_the_c_reference(golden_rules):
    positions = _golden_late(golden_rules, 0, 10)
    assert len(positions) >= 10 and max(ref.empties(a, b) for a, b in positions) == 10
    n_pass = n_rows = 0
    # (every position, none dropped: solve_bits is the cost, so the games are spread over worker processes)
    games = [(own, opp, i % 2, 64 - ref.empties(own, opp), 0, 128) for i, (own, opp) in enumerate(positions)]
    played = play_ref.play_out_many(games, workers=max(1, min(8, os.cpu_count() or 1)))
    for i, g in enumerate(played):
        rows = g["rows"]
        assert [r[0] for r in rows] == list(range(i % 2, g["n_turns"])) and g["n_turns"] % 2 == 0
        solved = [r for r in rows if r[3] == 3]
        for t, a, b, valid, move, score in rows:
            assert a & b == 0
            if valid == 3:
                assert (score, move) == orc.solve_endgame(a, b)[:2], (i, t)
                assert (ref.bit_legal(a, b) >> move) & 1
            else:
                assert (valid, move, score) == (0, -1, 0)
                n_pass += ref.bit_legal(a, b) == 0 and ref.bit_legal(b, a) != 0
        n_rows += len(solved)
        # under perfect play by both sides the value changes sides every turn, a pass included
        for x, y in zip(solved, solved[1:]):
            assert y[5] == (x[5] if (y[0] - x[0]) % 2 == 0 else -x[5]), (i, x[0], y[0])
        # the final position is over, and judged it is the first solved score's sign (own = the next mover)
        assert ref.bit_legal(g["own"], g["opp"]) == 0 and ref.bit_legal(g["opp"], g["own"]) == 0
        if solved:
            t0, score0 = solved[0][0], solved[0][5]
            final = ref.BitRules.score((g["own"], g["opp"])) * (1 if (g["n_turns"] - t0) % 2 == 0 else -1)
            assert final == score0
            z = orc.judge(orc.bits_to_state(g["own"], g["opp"]), 1 if (g["n_turns"] - t0) % 2 == 0 else 2)
            assert z == (score0 > 0) - (score0 < 0)
    assert n_rows > 50 and n_pass > 0


def test_play_ref_books():
    """The books on hand-built cases: max_turns cuts a game, a full board ends it at the next even turn, a pass
    after a pass ends a game that cannot fill the board."""
    own, opp = ref.late_positions(1, 5, 6, 6)
    own, opp = int(own[0]), int(opp[0])
    g = play_ref.play_out(own, opp, 50, 58, 0, 52)
    assert g["n_turns"] == 52 and len(g["rows"]) == 2
    full = 0xFFFFFFFFFFFFFFFF
    a = full & ~1
    g = play_ref.play_out(a & 0x00000000FFFFFFFF, a & ~0x00000000FFFFFFFF, 3, 63, 0, 128)
    if g["rows"][0][3] == 3:   # the last square is taken at the odd turn 3: stones 64, over at turn 4
        assert g["n_turns"] == 4
    # nobody can move: turn 2 passes, turn 3 passes again (stones = 64), the game is over at turn 4
    g = play_ref.play_out(0xFF, 0xFF00000000000000, 2, 16, 0, 128)
    assert [r[3] for r in g["rows"]] == [0, 0] and g["n_turns"] == 4 and (g["own"], g["opp"]) == (0xFF, 0xFF00000000000000)
    # ... and with the pass flag already set the first pass ends it: after the odd turn 3 at the latest
    g = play_ref.play_out(0xFF, 0xFF00000000000000, 3, 16, 1, 128)
    assert g["n_turns"] == 4 and len(g["rows"]) == 1
