"""Exact endgame references for the solver tests (iago_solve_endgame, include/iago_hip_serving.h).

One negamax alpha-beta search on two sets of rules:
  * OracleRules: the oracle's own rules (oracle.legal_actions / place_stone / judge on (8,8) boards, pinned to the
    reference by the golden fixtures) -- the slow, trusted one;
  * BitRules: a Python-int bitboard twin of the same rules -- fast enough for thousands of positions at <= 10 empties.
Game: a side with no legal move passes, the game ends when neither side can move, the score is #own - #opp at the end
(empty squares count for nobody).  `solve` returns (score, move): move = the LOWEST-indexed move that reaches the
score (-1: the side to move must pass, -2: the game is over).  wld=True scores the end of the game by its sign.
"""
import numpy as np

from oracle import oracle as orc

INF = 1000
FULL = 0xFFFFFFFFFFFFFFFF


def _sign(x):
    return (x > 0) - (x < 0)


class OracleRules(object):
    """pos = ((8,8) float32 board, colour to move)."""

    @staticmethod
    def moves(pos):
        return sorted(orc.legal_actions(pos[0], pos[1]))

    @staticmethod
    def play(pos, m):
        s = pos[0].copy()
        orc.place_stone(s, m, pos[1])
        return (s, 3 - pos[1])

    @staticmethod
    def pass_(pos):
        return (pos[0], 3 - pos[1])

    @staticmethod
    def score(pos):
        s, c = pos
        d = int(np.sum(s == c)) - int(np.sum(s == 3 - c))
        assert _sign(d) == orc.judge(s, c)
        return d


# (shift, mask of the squares a stone may come FROM without wrapping round a file) for the 8 directions
_DIRS = [(1, 0x7F7F7F7F7F7F7F7F), (-1, 0xFEFEFEFEFEFEFEFE), (8, FULL), (-8, FULL),
         (9, 0x7F7F7F7F7F7F7F7F), (7, 0xFEFEFEFEFEFEFEFE), (-7, 0x7F7F7F7F7F7F7F7F), (-9, 0xFEFEFEFEFEFEFEFE)]


def _sh(x, s):
    return ((x << s) & FULL) if s > 0 else (x >> -s)


def bit_legal(own, opp):
    empty = ~(own | opp) & FULL
    legal = 0
    for s, mask in _DIRS:
        t = _sh(own & mask, s) & opp
        for _ in range(5):
            t |= _sh(t & mask, s) & opp
        legal |= _sh(t & mask, s) & empty
    return legal


def bit_flips(own, opp, m):
    flips = 0
    for s, mask in _DIRS:
        run, x = 0, 1 << m
        while True:
            if not x & mask:
                run = 0
                break
            x = _sh(x, s)
            if x & opp:
                run |= x
            elif x & own:
                break
            else:
                run = 0
                break
        flips |= run
    return flips


class BitRules(object):
    """pos = (own, opp) Python ints, own = side to move."""

    @staticmethod
    def moves(pos):
        lm = bit_legal(*pos)
        return [a for a in range(64) if (lm >> a) & 1]

    @staticmethod
    def play(pos, m):
        own, opp = pos
        f = bit_flips(own, opp, m)
        return (opp & ~f, own | f | (1 << m))

    @staticmethod
    def pass_(pos):
        return (pos[1], pos[0])

    @staticmethod
    def score(pos):
        return bin(pos[0]).count("1") - bin(pos[1]).count("1")


def negamax(R, pos, alpha, beta, wld):
    """Fail-soft alpha-beta: exact inside (alpha, beta), a bound outside."""
    moves = R.moves(pos)
    if not moves:
        other = R.pass_(pos)
        if not R.moves(other):
            s = R.score(pos)
            return _sign(s) if wld else s
        return -negamax(R, other, -beta, -alpha, wld)
    best = -INF
    for m in moves:
        v = -negamax(R, R.play(pos, m), -beta, -max(alpha, best), wld)
        if v > best:
            best = v
            if best >= beta:
                break
    return best


def solve(R, pos, wld=False):
    """(score, move) of `pos` under perfect play; move: the lowest index reaching the score."""
    moves = R.moves(pos)
    if not moves:
        other = R.pass_(pos)
        if not R.moves(other):
            s = R.score(pos)
            return (_sign(s) if wld else s), -2
        v, _ = solve(R, other, wld)
        return -v, -1
    best, best_m = -INF, None
    for m in moves:   # ascending: a later move must beat the best strictly, so the window (best, INF) decides it
        v = -negamax(R, R.play(pos, m), -INF, -best, wld)
        if v > best:
            best, best_m = v, m
    return best, best_m


def solve_bits(own, opp, wld=False):
    return solve(BitRules, (int(own), int(opp)), wld)


def solve_state(state, color, wld=False):
    return solve(OracleRules, (np.asarray(state, np.float32).copy(), int(color)), wld)


def empties(own, opp):
    return 64 - bin(int(own) | int(opp)).count("1")


def late_positions(n, seed, lo, hi):
    """n positions (own, opp) with lo..hi empties from seeded uniform-random oracle playouts (cut at a random turn of
    that range; positions where the side to move must pass included)."""
    rs = np.random.RandomState(seed)
    own, opp = [], []
    g = 0
    while len(own) < n:
        _, _, tr = orc.random_playout(orc.initial_state(), 1, seed=seed, game_id=g)
        g += 1
        s, color = orc.initial_state(), 1
        cands = []
        for t, a in enumerate(tr + [None]):
            p1, p2 = orc.state_to_bits(s)
            e = empties(p1, p2)
            if lo <= e <= hi:
                cands.append((p1, p2) if color == 1 else (p2, p1))
            if a is None:
                break
            if a != -1:
                orc.place_stone(s, a, color)
            color = 3 - color
        if cands:
            o, p = cands[rs.randint(len(cands))]
            own.append(o)
            opp.append(p)
    return np.array(own, np.uint64), np.array(opp, np.uint64)


def golden_positions(trace, lo, hi):
    """The reference-recorded positions (tests/golden/rules.npz "trace": p1, p2, colour, ...) with lo..hi empties,
    from the side to move's point of view."""
    p1, p2, color = trace[:, 0], trace[:, 1], trace[:, 2]
    own = np.where(color == 1, p1, p2)
    opp = np.where(color == 1, p2, p1)
    e = np.array([empties(a, b) for a, b in zip(own, opp)])
    keep = (e >= lo) & (e <= hi)
    return own[keep], opp[keep]
