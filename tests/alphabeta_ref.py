"""The rule of the fixed-depth alpha-beta opponent and of its random openings (include/iago_hip_serving.h,
iago_alphabeta_moves / iago_random_moves) in a few lines of Python, on the bit rules of endgame_ref.py and the oracle's
Philox (pinned to the Random123 vectors in test_oracle_golden.py).

    search(own, opp, d):
        lo = legal(own, opp)
        if lo == 0:
            if legal(opp, own) == 0: return terminal(own, opp)      # game over, at any depth
            return -search(opp, own, d)                             # pass in place: costs no depth
        if d == 0: return eval(own, opp)
        return max over legal m of -search(play(own, opp, m), d - 1)

    terminal = 10000 sign(D) + 100 D, D = popcount(own) - popcount(opp)
    eval     = sum_k v_k (popcount(own & M_k) - popcount(opp & M_k)) + 8 (popcount(legal(own, opp)) - popcount(legal(opp, own)))

The root returns (score, move): move = the LOWEST-indexed move whose value equals the score, -1 where the mover must
pass (score: the negated value for the opponent), -2 where the game is over.  `minimax` is the rule with no pruning,
`alphabeta` the same value through fail-soft alpha-beta with the root's tie rule.

The opening draw: with K >= 1 legal moves the r-th lowest legal cell, r = (uint64(w) * K) >> 32, w = word t & 3 of
Philox4x32-10 on the counter (id_base + g mod id_mod, t >> 2, 0, 0), key = seed with its high word ^ 0x4F50454E."""
from oracle import oracle as orc

from .endgame_ref import bit_flips, bit_legal

OPENING_KEY = 0x4F50454E   # "OPEN"
WINDOW = 32767
CLASSES = ((100, 0x8100000000000081), (-20, 0x4281000000008142), (-50, 0x0042000000004200), (10, 0x2400810000810024),
           (5, 0x1800008181000018), (-2, 0x003C424242423C00), (-1, 0x00003C3C3C3C0000))


def _pc(x):
    return bin(x).count("1")


def terminal(own, opp):
    d = _pc(own) - _pc(opp)
    return 10000 * ((d > 0) - (d < 0)) + 100 * d


def evaluate(own, opp):
    return (sum(v * (_pc(own & m) - _pc(opp & m)) for v, m in CLASSES)
            + 8 * (_pc(bit_legal(own, opp)) - _pc(bit_legal(opp, own))))


def moves_of(own, opp):
    lm = bit_legal(own, opp)
    return [a for a in range(64) if (lm >> a) & 1]


def play(own, opp, m):
    f = bit_flips(own, opp, m)
    return opp & ~f, own | f | (1 << m)


def search(own, opp, d):
    """The rule, no pruning."""
    moves = moves_of(own, opp)
    if not moves:
        if not bit_legal(opp, own):
            return terminal(own, opp)
        return -search(opp, own, d)
    if d == 0:
        return evaluate(own, opp)
    return max(-search(*play(own, opp, m), d - 1) for m in moves)


def minimax(own, opp, depth):
    """(score, move) by the plain rule: every root move's exact value, the first maximum."""
    own, opp = int(own), int(opp)
    moves = moves_of(own, opp)
    if not moves:
        if not bit_legal(opp, own):
            return terminal(own, opp), -2
        return -search(opp, own, depth), -1
    values = [-search(*play(own, opp, m), depth - 1) for m in moves]
    best = max(values)
    return best, moves[values.index(best)]


def _ab(own, opp, d, alpha, beta):
    """Fail-soft alpha-beta: exact inside (alpha, beta), a bound outside."""
    moves = moves_of(own, opp)
    if not moves:
        if not bit_legal(opp, own):
            return terminal(own, opp)
        return -_ab(opp, own, d, -beta, -alpha)
    if d == 0:
        return evaluate(own, opp)
    best = -WINDOW - 1
    for m in moves:
        v = -_ab(*play(own, opp, m), d - 1, -beta, -max(alpha, best))
        if v > best:
            best = v
            if best >= beta:
                break
    return best


def alphabeta(own, opp, depth):
    """(score, move) with pruning: ascending root moves, a later one must beat the best strictly, so the window
    (best, WINDOW) decides it."""
    own, opp = int(own), int(opp)
    moves = moves_of(own, opp)
    if not moves:
        if not bit_legal(opp, own):
            return terminal(own, opp), -2
        return -_ab(opp, own, depth, -WINDOW, WINDOW), -1
    best, best_m = -WINDOW - 1, None
    for m in moves:
        v = -_ab(*play(own, opp, m), depth - 1, -WINDOW, -max(best, -WINDOW))
        if v > best:
            best, best_m = v, m
    return best, best_m


def nodes_in_tree(own, opp, d):
    """True when some node below (own, opp) within depth d must pass (the game going on)."""
    moves = moves_of(own, opp)
    if not moves:
        return bool(bit_legal(opp, own))
    if d == 0:
        return False
    return any(nodes_in_tree(*play(own, opp, m), d - 1) for m in moves)


def pass_inside(own, opp, depth):
    """True when the root can move and a node of its tree to `depth` (leaves included) must pass."""
    own, opp = int(own), int(opp)
    return bool(bit_legal(own, opp)) and nodes_in_tree(own, opp, depth)


def _sq(r, c):
    return 1 << (8 * r + c)


_FULL = 0xFFFFFFFFFFFFFFFF
_ROW0 = 0xFFFFFFFF00000000 | 0xFF
# hand-made boards (own, opp): a full board; one empty that only the mover / only the other side can take; a root that
# must pass before the opponent's last move; two games that are over with many empties; a tie between two moves
HAND_MADE = (
    (_ROW0, _FULL & ~_ROW0),
    (_FULL & ~_sq(0, 0) & ~_sq(1, 0), _sq(1, 0)),
    (_sq(1, 0), _FULL & ~_sq(0, 0) & ~_sq(1, 0)),
    (_sq(0, 1), sum(_sq(0, c) for c in range(2, 8))),
    (sum(_sq(0, c) for c in range(2, 8)), _sq(0, 1)),
    (_sq(3, 3), _sq(5, 5)),
    (_sq(3, 3) | _sq(0, 0), _sq(5, 5)),
    (_sq(0, 3), _sq(0, 2) | _sq(0, 4)),
)


def position_set():
    """The 48 positions of the reference's own tests and of the kernel's: seeded random-play positions from 9 to 56
    empties, late ones (0 to 8 empties: roots that must pass, finished games, passes inside the tree) and HAND_MADE.
    Returns two lists of Python ints."""
    from .endgame_ref import late_positions
    own, opp = [], []
    for n, seed, lo, hi in ((24, 5, 9, 56), (16, 4, 0, 8)):   # (seed 4: three roots that must pass, two finished games)
        o, p = late_positions(n, seed, lo, hi)
        own += [int(x) for x in o]
        opp += [int(x) for x in p]
    own += [a for a, _ in HAND_MADE]
    opp += [b for _, b in HAND_MADE]
    return own, opp


def kind_counts(own, opp, depth):
    """(roots that must pass, finished games, positions with a pass inside the tree to `depth`) of a position set."""
    must_pass = sum(1 for a, b in zip(own, opp) if not bit_legal(a, b) and bit_legal(b, a))
    over = sum(1 for a, b in zip(own, opp) if not bit_legal(a, b) and not bit_legal(b, a))
    inside = sum(1 for a, b in zip(own, opp) if pass_inside(a, b, depth))
    return must_pass, over, inside


def word(seed, game_id, turn):
    """The raw 32-bit word of (seed, id, turn)."""
    key = (int(seed) ^ (OPENING_KEY << 32)) & 0xFFFFFFFFFFFFFFFF
    return int(orc.philox(key, int(game_id) & 0xFFFFFFFF, int(turn) >> 2, 0, 0)[int(turn) & 3])


def opening_id(g, id_base, id_mod):
    return (int(id_base) + int(g) % int(id_mod)) & 0xFFFFFFFF


def random_index(w, K):
    return (int(w) * int(K)) >> 32


def random_move(own, opp, seed, g, id_base, id_mod, turn):
    """The opening move of game g's mover at `turn`; -1 where it has no legal move."""
    moves = moves_of(int(own), int(opp))
    if not moves:
        return -1
    return moves[random_index(word(seed, opening_id(g, id_base, id_mod), turn), len(moves))]
