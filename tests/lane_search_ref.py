"""The VISITING ORDER of the lane-per-position alpha-beta searches (iago_solve_endgame, iago_play_endgame,
iago_alphabeta_moves and the job lanes of iago_alphabeta_moves_split) as a plain recursion with a node counter.

endgame_ref.py and alphabeta_ref.py state the VALUE of a search; `nodes` is the one output that also shows the order in
which the kernel visits the tree, so it is restated here, rule for rule.  A deterministic recursion visits the nodes an
explicit stack visits:

  * entering a node counts one.  A mover without a legal move whose opponent has none either ends the game (the
    terminal value, move -2); otherwise it PASSES IN PLACE: the sides swap, the window is negated, the node goes on as
    the opponent's and negates its value when it returns -- no second node, no level used;
  * solver: a node with one level (= one empty) left is counted directly: its one move is played and valued as the end
    of the game, one more node;
  * yardstick: the children of a node with one level left are LEAVES, valued in the parent (the evaluation, or the
    terminal value when neither side can move), one node each -- a leaf whose mover must pass is not looked at again;
  * move order.  Solver: above 6 empties the untried move with the fewest replies for the opponent, else the lowest
    index.  Yardstick: a corner (the lowest one) first; without one, with at least 3 levels left, the fewest replies;
    else the lowest index.  Ties in the replies go to the lowest index;
  * fail-soft alpha-beta: best = max(best, v), alpha = max(alpha, best), the untried moves are dropped at alpha >= beta;
  * the root (unless it passed: then it is a node like any other and its move is -1) keeps its window and searches a
    move that could tie the best value with a LOWER index with alpha = best - 1, a higher one with alpha = best, so a
    tie comes back exact and `move` is the lowest-indexed move of the best value; a move whose window would be empty is
    not searched.

`levels` is the root's remaining levels: its empties for the solver, the depth for the yardstick.
"""
from . import alphabeta_ref as ab
from .endgame_ref import bit_flips, bit_legal

CORNERS = 0x8100000000000081


def _pc(x):
    return bin(x).count("1")


def _lowest(x):
    return (x & -x).bit_length() - 1


def _play(own, opp, m):
    f = bit_flips(own, opp, m)
    return opp & ~f, own | f | (1 << m)


def _fewest_replies(own, opp, moves):
    best_m, best_mob = None, 65
    while moves:
        m = _lowest(moves)
        moves &= moves - 1
        mob = _pc(bit_legal(*_play(own, opp, m)))
        if mob < best_mob:
            best_m, best_mob = m, mob
    return best_m


class Solver(object):
    """iago_solve_endgame / iago_play_endgame: the final disc difference (wld: its sign)."""
    count_last = True       # a node with one level left is counted directly
    leaf_children = False

    def __init__(self, wld=False):
        self.wld = wld
        self.neg_inf = -100
        self.window = 1 if wld else 65

    def terminal(self, own, opp):
        d = _pc(own) - _pc(opp)
        return (d > 0) - (d < 0) if self.wld else d

    @staticmethod
    def pick(own, opp, moves, levels):
        return _fewest_replies(own, opp, moves) if levels > 6 else _lowest(moves)


class Yardstick(object):
    """iago_alphabeta_moves and the jobs of iago_alphabeta_moves_split."""
    count_last = False
    leaf_children = True    # the children of a node with one level left are valued in the parent
    neg_inf = -32768
    window = 32767
    terminal = staticmethod(ab.terminal)

    @staticmethod
    def leaf(own, opp):
        if not bit_legal(own, opp) and not bit_legal(opp, own):
            return ab.terminal(own, opp)
        return ab.evaluate(own, opp)

    @staticmethod
    def pick(own, opp, moves, levels):
        if moves & CORNERS:
            return _lowest(moves & CORNERS)
        return _fewest_replies(own, opp, moves) if levels >= 3 else _lowest(moves)


def _visit(R, own, opp, levels, alpha, beta, root, count):
    """(value, root move) of the node for its mover; count[0] += the nodes visited."""
    count[0] += 1
    legal = bit_legal(own, opp)
    sign = 1
    if not legal:
        legal = bit_legal(opp, own)
        if not legal:
            return R.terminal(own, opp), -2
        own, opp, alpha, beta, sign, root = opp, own, -beta, -alpha, -1, False   # the pass in place
    if R.count_last and levels == 1:
        m = _lowest(legal)
        count[0] += 1
        cown, copp = _play(own, opp, m)
        return sign * R.terminal(copp, cown), (m if sign > 0 else -1)
    moves, best = legal, R.neg_inf
    best_m = 64 if root else -1
    while moves:
        m = R.pick(own, opp, moves, levels)
        moves &= ~(1 << m)
        a_child = alpha
        if root and best > R.neg_inf:
            a_child = max(alpha, best - 1 if m < best_m else best)
        if a_child >= beta:
            continue
        cown, copp = _play(own, opp, m)
        if R.leaf_children and levels <= 1:
            count[0] += 1
            v = -R.leaf(cown, copp)
        else:
            v = -_visit(R, cown, copp, levels - 1, -beta, -a_child, False, count)[0]
        if root:
            if v > best or (v == best and m < best_m):
                best, best_m = v, m
        else:
            best = max(best, v)
            alpha = max(alpha, best)
            if alpha >= beta:
                break
    return sign * best, best_m


def _search(R, own, opp, levels):
    own, opp = int(own), int(opp)
    count = [0]
    v, m = _visit(R, own, opp, levels, -R.window, R.window, True, count)
    return v, m, count[0]


def solve(own, opp, wld=False):
    """(score, move, nodes) of iago_solve_endgame on one admitted position."""
    return _search(Solver(wld), own, opp, 64 - _pc(int(own) | int(opp)))


def alphabeta(own, opp, depth):
    """(score, move, nodes) of iago_alphabeta_moves on one position (of a job at its depth left)."""
    return _search(Yardstick, own, opp, int(depth))
