"""The rule of iago_replay_sample (include/iago_hip_training.h) in a few lines of numpy, on the oracle's Philox (pinned
to the Random123 vectors in test_oracle_golden.py).  Output row j of a minibatch keyed by (seed, step), out of a window
whose slots 0 .. count-1 are filled:

    c     Philox4x32-10 on the counter (j, step, 0, 0), key = seed with its high word ^ 0x52504C59
    slot  (uint64(c[0]) * count) >> 32
    sym   c[1] & 7

and variant k of the board's symmetries, in ops.augment8's order: 0 the identity, 1 .. 3 successive counter-clockwise
quarter turns (cell (y, x) -> (7 - x, y)), 4 the transpose of variant 3, 5 .. 7 three more turns.  With m_k the cell
map: the boards have bit m_k(a) where the source has bit a, pi_out[m_k(a)] = pi[a], move_out = m_k(move) (-1 stays)."""
import numpy as np

from oracle import oracle as orc

REPLAY_KEY = 0x52504C59   # "RPLY"


def draw(seed, step, j, count):
    """(slot, sym) of output row j."""
    key = (int(seed) ^ (REPLAY_KEY << 32)) & 0xFFFFFFFFFFFFFFFF
    c = orc.philox(key, int(j) & 0xFFFFFFFF, int(step) & 0xFFFFFFFF, 0, 0)
    return (int(c[0]) * int(count)) >> 32, int(c[1]) & 7


def _turn(a):
    y, x = divmod(a, 8)
    return (7 - x) * 8 + y


def _transpose(a):
    y, x = divmod(a, 8)
    return x * 8 + y


def cell_map(k):
    """m_k as 64 integers: cell a of the source is cell cell_map(k)[a] of variant k."""
    cells = list(range(64))
    for i in range(1, int(k) + 1):
        cells = [_transpose(a) if i == 4 else _turn(a) for a in cells]
    return cells


def _bits(x, m):
    x = int(x) & 0xFFFFFFFFFFFFFFFF
    return sum(1 << m[a] for a in range(64) if (x >> a) & 1)


def apply(own, opp, pi, move, k):
    """Variant k of one row: (own, opp) as Python ints (unsigned 64-bit), pi as 64 integers, the move."""
    m = cell_map(k)
    pi = np.asarray(pi).reshape(64)
    out = np.zeros(64, dtype=pi.dtype)
    out[m] = pi
    return _bits(own, m), _bits(opp, m), out, (int(move) if int(move) < 0 else m[int(move)])
