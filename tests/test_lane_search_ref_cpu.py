"""The restatement of the lane searches' visiting order (tests/lane_search_ref.py) against the value references: its
(score, move) is alphabeta_ref.alphabeta's and endgame_ref.solve_bits', and its node counts are the ones that can be
counted by hand."""
import pytest

from . import alphabeta_ref as ab
from . import endgame_ref as er
from . import lane_search_ref as ls


@pytest.fixture(scope="module")
def positions():
    return ab.position_set()


@pytest.fixture(scope="module")
def late():
    own, opp = er.late_positions(48, 23, 0, 9)
    return [int(a) for a in own], [int(b) for b in opp]


@pytest.mark.parametrize("depth", [1, 2, 3, 4])
def test_yardstick_equals_the_value_reference(positions, depth):
    own, opp = positions
    for a, b in zip(own, opp):
        assert ls.alphabeta(a, b, depth)[:2] == ab.alphabeta(a, b, depth), (hex(a), hex(b))


@pytest.mark.parametrize("wld", [False, True])
def test_solver_equals_the_value_reference(positions, late, wld):
    own, opp = late
    # (the late and hand-made boards of the yardstick's set too: roots that must pass, finished games, a full board)
    own, opp = own + list(positions[0][24:]), opp + list(positions[1][24:])
    kinds = set()
    for a, b in zip(own, opp):
        if er.empties(a, b) > 9:
            continue
        got = ls.solve(a, b, wld)
        assert got[:2] == er.solve_bits(a, b, wld), (hex(a), hex(b))
        kinds.add(min(got[1], 0))
    assert kinds == {0, -1, -2}


def test_node_counts_that_can_be_counted_by_hand(positions):
    own, opp = positions
    for a, b in zip(own, opp):
        lo, lp = er.bit_legal(a, b), er.bit_legal(b, a)
        # depth 1: the root and a leaf per move of whoever moves there (nothing is cut off: every value lies inside
        # the root's window); a finished game is its root alone
        moves = bin(lo or lp).count("1")
        assert ls.alphabeta(a, b, 1)[2] == 1 + moves, (hex(a), hex(b))
        if moves == 0:
            assert ls.solve(a, b)[2] == 1
        elif er.empties(a, b) == 1:
            assert ls.solve(a, b)[2] == 2   # the last empty is counted directly: the root and the full board
