"""The root rules BEST and ALL of the lane-per-position search (iago_solve_endgame_moves, iago_play_endgame_moves) as a
plain recursion on top of lane_search_ref: everything below the root is lane_search_ref._visit, node for node.

The root (unless it must pass: then it is a node like any other, move -1, the empty set; a finished game: move -2, the
empty set) keeps lane_search_ref's move order and window and differs from its rule LOWEST in two places only:

  * BEST: every move searched after the first gets a_child = max(alpha, best - 1), whatever its index; a move whose
    window is empty is not searched.  A value above best replaces the set with that move, a value equal to best adds the
    move to it -- with fail-soft returns such a value lies inside (a_child, beta), so it is exact.  Under WLD with
    best == 1 the later moves are searched with the window (0, 1);
  * ALL: the root's alpha never rises: every move is searched with the full window and its value recorded; the set is
    the argmax.

A root with one empty is counted directly (two nodes): its one move is the set and that move's value the score.
`move` is the lowest set bit of the set.
"""
from . import lane_search_ref as ls
from .endgame_ref import bit_legal

BEST, ALL = "best", "all"


def solve_moves(own, opp, wld=False, rule=BEST, trace=None):
    """(score, move, nodes, best, scores) of iago_solve_endgame_moves on one admitted position.  best: the set as an
    int; scores: {move: value} under ALL, None under BEST.  trace (a list, BEST): gets (move, value, a_child, beta) of
    every move searched at the root."""
    assert rule in (BEST, ALL)
    own, opp = int(own), int(opp)
    R = ls.Solver(wld)
    levels = 64 - ls._pc(own | opp)
    alpha, beta = -R.window, R.window
    count = [0]
    legal = bit_legal(own, opp)
    if not legal:      # a pass root or a finished game: lane_search_ref's node
        v, m = ls._visit(R, own, opp, levels, alpha, beta, True, count)
        return v, m, count[0], 0, ({} if rule == ALL else None)
    count[0] += 1
    if levels == 1:    # counted directly
        m = ls._lowest(legal)
        count[0] += 1
        cown, copp = ls._play(own, opp, m)
        v = R.terminal(copp, cown)
        return v, m, count[0], 1 << m, ({m: v} if rule == ALL else None)
    moves, best, best_set, scores = legal, R.neg_inf, 0, {}
    while moves:
        m = R.pick(own, opp, moves, levels)
        moves &= ~(1 << m)
        a_child = alpha
        if rule == BEST and best > R.neg_inf:
            a_child = max(alpha, best - 1)
        if a_child >= beta:
            continue
        cown, copp = ls._play(own, opp, m)
        v = -ls._visit(R, cown, copp, levels - 1, -beta, -a_child, False, count)[0]
        if trace is not None:
            trace.append((m, v, a_child, beta))
        scores[m] = v
        if v > best:
            best, best_set = v, 1 << m
        elif v == best:
            best_set |= 1 << m
    return best, ls._lowest(best_set), count[0], best_set, (scores if rule == ALL else None)


# hand-made roots: (name, own, opp)
def hand_made():
    """A full board, a position where neither side can move, positions with one and two empties."""
    full = (0x00000000FFFFFFFF, 0xFFFFFFFF00000000)
    # neither side can move with two empties left (a1, b1 = bits 0, 1): the opponent's one disc (g8 = bit 62) is on no
    # line through them, the mover has nothing to bracket
    dead = (0xFFFFFFFFFFFFFFFF & ~(1 << 62) & ~0x3, 1 << 62)
    # one empty (a1 = bit 0): the mover on the rest of row 1's far end, the opponent between
    one = (0xFFFFFFFFFFFFFF80, 0x000000000000007E)
    # two empties (a1, h1 = bits 0, 7), both legal and mirror images of each other: the opponent holds rows 2 .. 7 of
    # the columns a and h, the mover everything else -- two optimal moves
    two_opp = sum(1 << (8 * r + c) for r in range(1, 7) for c in (0, 7))
    two = (0xFFFFFFFFFFFFFFFF & ~two_opp & ~0x81, two_opp)
    # one empty where the mover must pass and the opponent fills it
    one_pass = (0x000000000000007E, 0xFFFFFFFFFFFFFF80)
    return [("full", ) + full, ("dead", ) + dead, ("one", ) + one, ("two", ) + two, ("one_pass", ) + one_pass]
