"""The rule of exploring self-play (include/iago_hip_serving.h, iago_mcts_search_explore) in a few lines of numpy, on
the oracle's Philox (pinned to the Random123 vectors in test_oracle_golden.py).  At a searched turn t < explore_turns
of the game with global id G:

    n[a]  the visit counts of the root's children by cell (the turn's `pi` row), N their sum
    w     word t & 3 of Philox4x32-10 on the counter (G, t >> 2, 0, 0), key = seed with its high word ^ 0x4558504C
    r     (uint64(w) * N) >> 32
    move  the lowest cell a with sum_{b <= a} n[b] > r

N == 0: the most visited child's first-maximum rule -- with every count 0, the lowest legal cell."""
import numpy as np

from oracle import oracle as orc

EXPLORE_KEY = 0x4558504C   # "EXPL"


def word(seed, game_id, turn):
    """The raw 32-bit word of (seed, global game id, turn)."""
    key = (int(seed) ^ (EXPLORE_KEY << 32)) & 0xFFFFFFFFFFFFFFFF
    return int(orc.philox(key, int(game_id) & 0xFFFFFFFF, int(turn) >> 2, 0, 0)[int(turn) & 3])


def draw_from_word(n, w, legal=None):
    """The move for the visit row n (64 counts) and the word w.  legal: the mover's legal cells, read when N == 0 only
    (None there: the row alone cannot say, None is returned)."""
    n = np.asarray(n, dtype=np.int64).reshape(64)
    assert (n >= 0).all() and 0 <= int(w) <= 0xFFFFFFFF
    total = int(n.sum())
    if total == 0:
        return None if legal is None else int(min(legal))
    r = (int(w) * total) >> 32
    return int(np.argmax(np.cumsum(n) > r))


def draw(n, seed, game_id, turn, legal=None):
    return draw_from_word(n, word(seed, game_id, turn), legal)
