"""The restatement of the root rules BEST and ALL (tests/endgame_moves_ref.py) against the C reference's per-move
values (oracle.root_values) and against the rule LOWEST (lane_search_ref.solve), on the 64 late positions the device
tests use and on hand-made roots; the bindings of the two entry points without a device."""
import ctypes as C
import os
import re

import pytest

from iago_amd import _lib
from oracle import oracle as orc

from . import endgame_moves_ref as mr
from . import endgame_ref as er
from . import lane_search_ref as ls


@pytest.fixture(scope="module")
def late():
    own, opp = er.late_positions(64, 29, 2, 10)
    return [int(a) for a in own], [int(b) for b in opp]


@pytest.fixture(scope="module")
def values(late):
    """wld -> [{move: value}] of the C reference."""
    own, opp = late
    return {wld: [orc.root_values(a, b, wld=wld) for a, b in zip(own, opp)] for wld in (False, True)}


def _argmax(vals):
    top = max(vals.values())
    return top, sum(1 << m for m, v in vals.items() if v == top)


@pytest.mark.parametrize("wld", [False, True])
@pytest.mark.parametrize("rule", [mr.BEST, mr.ALL])
def test_rules_against_the_oracle(late, values, wld, rule):
    own, opp = late
    ties = passes = finished = 0
    for a, b, vals in zip(own, opp, values[wld]):
        trace = []
        score, move, nodes, best, scores = mr.solve_moves(a, b, wld, rule, trace)
        assert (score, move) == ls.solve(a, b, wld)[:2], (hex(a), hex(b))
        if not vals:            # no move: a pass root or a finished game
            assert best == 0 and move in (-1, -2) and not scores
            passes += move == -1
            finished += move == -2
            continue
        top, want = _argmax(vals)
        assert (score, best) == (top, want), (hex(a), hex(b))
        assert move == ls._lowest(best)
        ties += bin(best).count("1") >= 2
        if rule == mr.ALL:
            assert scores == vals, (hex(a), hex(b))
            assert nodes >= ls.solve(a, b, wld)[2]
        else:
            assert scores is None
            for m, v, a_child, beta in trace:
                if v == score:
                    # a tie came back inside its window, or at an end of the value range where a bound is the value:
                    # under WLD the window (0, 1) holds no value, a win comes back as 1 >= beta and nothing lies above
                    top_v = 1 if wld else 64
                    assert a_child < v < beta or v == -top_v or (a_child < v and v == top_v), (hex(a), hex(b), m)
                    assert vals[m] == v
                else:
                    assert v < score and vals[m] <= v
    # the conditions of the set: the tie paths cannot drop out unnoticed
    assert (ties, passes, finished) == ((41 if wld else 9), 3, 0)


def test_node_counts_of_the_set():
    """The figures the feature was sized with: plain / BEST / ALL nodes over the set."""
    own, opp = er.late_positions(64, 29, 2, 10)
    for wld, want in ((False, (97388, 106256, 212211)), (True, (18715, 45124, 49905))):
        got = [0, 0, 0]
        for a, b in zip(own, opp):
            got[0] += ls.solve(a, b, wld)[2]
            got[1] += mr.solve_moves(a, b, wld, mr.BEST)[2]
            got[2] += mr.solve_moves(a, b, wld, mr.ALL)[2]
        assert tuple(got) == want


@pytest.mark.parametrize("wld", [False, True])
def test_hand_made_roots(wld):
    rows = {name: (a, b) for name, a, b in mr.hand_made()}
    assert sorted(rows) == ["dead", "full", "one", "one_pass", "two"]
    for name, (a, b) in rows.items():
        assert a & b == 0
        for rule in (mr.BEST, mr.ALL):
            score, move, nodes, best, scores = mr.solve_moves(a, b, wld, rule)
            assert (score, move) == ls.solve(a, b, wld)[:2]
            assert nodes == ls.solve(a, b, wld)[2] or name == "two"   # (a root with a choice searches more)
            vals = orc.root_values(a, b, wld=wld)
            if name in ("full", "dead"):
                assert (move, best, nodes) == (-2, 0, 1) and not vals
            elif name == "one_pass":
                assert (move, best, nodes) == (-1, 0, 2) and not vals
            else:
                assert best == _argmax(vals)[1] and score == _argmax(vals)[0] and move == ls._lowest(best)
                if rule == mr.ALL:
                    assert scores == vals
    assert er.empties(*rows["full"]) == 0 and er.empties(*rows["one"]) == 1 and er.empties(*rows["two"]) == 2
    assert er.empties(*rows["dead"]) == 2 and not er.bit_legal(*rows["dead"]) and not er.bit_legal(*rows["dead"][::-1])
    # two empties, both moves optimal
    assert mr.solve_moves(*rows["two"], wld, mr.BEST)[3] == mr.solve_moves(*rows["two"], wld, mr.ALL)[3] == 0x81
    # one empty: the one move is the set and its value the score, the root and the full board are the nodes
    a, b = rows["one"]
    assert mr.solve_moves(a, b, wld, mr.ALL) == (1 if wld else 64, 0, 2, 1, {0: 1 if wld else 64})


def test_header_and_bindings():
    """Both entry points are declared in the serving header, bound, and the mirrors have the C structs' sizes."""
    here = os.path.dirname(os.path.abspath(__file__))
    text = open(os.path.join(here, "..", "include", "iago_hip_serving.h")).read()
    declared = set(re.findall(r"IAGO_API[^;(]*?\b(iago_\w+)\s*\(", text))
    L = _lib.lib()
    for name in ("iago_solve_endgame_moves", "iago_play_endgame_moves"):
        assert name in declared and name in _lib.SERVING_SYMBOLS and hasattr(L, name), name
    assert C.sizeof(_lib.EndgameMovesArgs) == 8 * 3 + 4 * 4 + 8 * 7 + 8 * 4
    assert C.sizeof(_lib.PlayEndgameMovesArgs) == C.sizeof(_lib.PlayEndgameArgs) + 8 + 8 * 4
    assert L.iago_abi_version() == 13
    for name, value in (("IAGO_ENDGAME_MOVES_BEST", _lib.ENDGAME_MOVES_BEST), ("IAGO_ENDGAME_MOVES_ALL", _lib.ENDGAME_MOVES_ALL),
                        ("IAGO_ENDGAME_NO_MOVE", _lib.ENDGAME_NO_MOVE)):
        assert int(re.search(r"#define %s \(?(-?\d+)\)?" % name, text).group(1)) == value


def test_host_side_refusals_need_no_device():
    """What is refused before anything touches the device: null args, null pointers, modes, moves, ranges, reserved."""
    L = _lib.lib()

    def refused(a, what):
        assert L.iago_solve_endgame_moves(C.byref(a), None) == _lib.IAGO_ERR_INVALID
        msg = L.iago_last_error().decode()
        assert msg.startswith("iago_solve_endgame_moves: ") and what in msg, msg

    def args(**kw):
        a = _lib.EndgameMovesArgs()
        buf = C.create_string_buffer(64)   # never read: every call below is refused first
        p = C.cast(buf, C.c_void_p)
        for k in ("own", "opp", "score", "move", "nodes", "solved", "best", "ctl"):
            setattr(a, k, p)
        a._keep = buf
        a.n, a.mode, a.moves, a.max_empties, a.time_limit_ms = 1, 0, 0, 8, 1000
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    assert L.iago_solve_endgame_moves(None, None) == _lib.IAGO_ERR_INVALID
    for k in ("own", "opp", "score", "move", "nodes", "solved", "best", "ctl"):
        refused(args(**{k: None}), "null pointer")
    refused(args(n=-1), "negative n")
    refused(args(mode=2), "mode must be")
    refused(args(moves=2), "moves must be")
    refused(args(moves=-1), "moves must be")
    refused(args(move_score=args().own), "must be NULL under IAGO_ENDGAME_MOVES_BEST")
    refused(args(moves=_lib.ENDGAME_MOVES_ALL), "required under IAGO_ENDGAME_MOVES_ALL")
    refused(args(max_empties=21), "max_empties")
    refused(args(max_empties=-1), "max_empties")
    refused(args(time_limit_ms=0), "time_limit_ms")
    refused(args(time_limit_ms=_lib.ENDGAME_MAX_TIME_MS + 1), "time_limit_ms")
    for i in range(4):
        a = args()
        a.reserved[i] = 1
        refused(a, "reserved fields must be 0")

    m = _lib.PlayEndgameMovesArgs()
    assert L.iago_play_endgame_moves(None, None) == _lib.IAGO_ERR_INVALID
    assert L.iago_play_endgame_moves(C.byref(m), None) == _lib.IAGO_ERR_INVALID   # no ctl
    assert L.iago_last_error().decode().startswith("iago_play_endgame_moves: null pointer")
