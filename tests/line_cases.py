"""Every content of every board line, and the rules by their plain definition.

The cases.  A line is a row, a column or a diagonal of at least 3 cells; a cell of it is empty (0), the mover's (1) or
the opponent's (2), so a line of k cells has 3^k contents.  `cases()` puts every content on every line: 16 lines of 8
cells and two diagonal directions of 3 + 4 + 5 + 6 + 7 + 8 + 7 + 6 + 5 + 4 + 3 cells, 16 x 6561 + 2 x 13,095 = 131,166
positions.  Bare (no seed) the rest of the board is empty; with a seed every cell off the line is empty with probability
1/2 and otherwise the mover's or the opponent's with equal chance.

The order, fixed: line 0 .. 37 of `all_lines()` (rows 0 .. 7, columns 0 .. 7, the diagonals row - col = -5 .. 5, the
anti-diagonals row + col = 2 .. 12, each listed from its top cell down, a row from its left cell); within a line the
contents in ascending code, code = sum of state(cell j of the line) * 3^j.  So case `line_first()[l] + code` is content
`code` on line l, in both variants.

The reference.  `reference(own, opp)` is the rule as the game states it: from an empty cell, in each of the 8
directions, walk outwards cell by cell over a run of the opponent's stones; where the mover's stone ends the run the
run is turned.  It is vectorised over the POSITIONS only -- a cell of the board is one bit per position, a bit vector
over the batch -- and loops over cells, directions and steps in Python, so no board is ever shifted, masked, flooded,
carried through or reversed: nothing here can share a mistake with a bitboard kernel.  `legal` = empty and turns a
stone.  `tests/test_line_cases_cpu.py` holds it against the C oracle.

Bit a of a board is cell a = row * 8 + col; own = the side to move.  The arrays `cases` and `reference_of` return are
computed once per process and are read-only."""
import functools

import numpy as np

N_CASES = 16 * 3 ** 8 + 2 * (2 * (3 ** 3 + 3 ** 4 + 3 ** 5 + 3 ** 6 + 3 ** 7) + 3 ** 8)   # 131,166
NOISE_SEED = 20260   # the noisy variant of the tests
VARIANTS = {"bare": None, "noisy": NOISE_SEED}
DIRECTIONS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))
_CELLS = np.arange(64, dtype=np.uint64)
_ONE = np.uint64(1)


def all_lines():
    """The 38 lines of at least 3 cells, as lists of cells."""
    rows = [[r * 8 + c for c in range(8)] for r in range(8)]
    cols = [[r * 8 + c for r in range(8)] for c in range(8)]
    diag = [[r * 8 + (r - d) for r in range(8) if 0 <= r - d < 8] for d in range(-5, 6)]
    anti = [[r * 8 + (s - r) for r in range(8) if 0 <= s - r < 8] for s in range(2, 13)]
    return rows + cols + diag + anti


def line_first():
    """The index of every line's first case (its content 0), and the total as the last entry."""
    return np.concatenate([[0], np.cumsum([3 ** len(l) for l in all_lines()])]).astype(np.int64)


def line_masks():
    """(38,) uint64: the cells of every line."""
    return np.array([sum(1 << c for c in l) for l in all_lines()], dtype=np.uint64)


def code_of(states):
    """The content code of a line's cell states, first cell first."""
    return sum(int(s) * 3 ** j for j, s in enumerate(states))


def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


@functools.lru_cache(maxsize=None)
def cases(noise_seed=None):
    """(own, opp, line_id): uint64, uint64, int64 arrays of N_CASES entries in the documented order."""
    own, opp, line_id = [], [], []
    for l, cells in enumerate(all_lines()):
        k = len(cells)
        digit = (np.arange(3 ** k, dtype=np.int64)[:, None] // 3 ** np.arange(k, dtype=np.int64)) % 3   # [content, j]
        bit = np.array([1 << c for c in cells], dtype=np.uint64)
        own.append(((digit == 1) * bit).sum(axis=1, dtype=np.uint64))
        opp.append(((digit == 2) * bit).sum(axis=1, dtype=np.uint64))
        line_id.append(np.full(3 ** k, l, dtype=np.int64))
    own, opp, line_id = np.concatenate(own), np.concatenate(opp), np.concatenate(line_id)
    on_line = line_masks()[line_id]
    assert not (own & ~on_line).any() and not (opp & ~on_line).any()
    if noise_seed is not None:
        rs = np.random.RandomState(noise_seed)
        line_own, line_opp = own.copy(), opp.copy()
        for lo in range(0, len(own), 16384):        # 0, 1: empty; 2: the mover's; 3: the opponent's
            draw = rs.randint(0, 4, size=(len(own[lo:lo + 16384]), 64))
            off = ~on_line[lo:lo + 16384]
            own[lo:lo + 16384] |= ((draw == 2) * (_ONE << _CELLS)).sum(axis=1, dtype=np.uint64) & off
            opp[lo:lo + 16384] |= ((draw == 3) * (_ONE << _CELLS)).sum(axis=1, dtype=np.uint64) & off
        assert np.array_equal(own & on_line, line_own) and np.array_equal(opp & on_line, line_opp)   # the line is as it was
    assert not (own & opp).any()
    assert len(own) == N_CASES
    return _frozen(own, opp, line_id)


# ------------------------------------------------------------------------------------------------ the reference
def _cell_vectors(x):
    """Board array -> 64 bit vectors over the positions (packed, 8 positions a byte): entry c holds cell c of every board."""
    return [np.packbits(((x >> np.uint64(c)) & _ONE).astype(np.uint8)) for c in range(64)]


def _ray(cell, step):
    """The cells outwards from `cell` (itself not included) in direction `step`, to the edge."""
    r, c = divmod(cell, 8)
    out = []
    while True:
        r, c = r + step[0], c + step[1]
        if not (0 <= r < 8 and 0 <= c < 8):
            return out
        out.append(r * 8 + c)


def _walk(own, opp, want_flips):
    own, opp = np.ascontiguousarray(own, dtype=np.uint64), np.ascontiguousarray(opp, dtype=np.uint64)
    assert own.shape == opp.shape and own.ndim == 1
    n = len(own)
    mine, theirs = _cell_vectors(own), _cell_vectors(opp)
    empty = [~(a | b) for a, b in zip(mine, theirs)]   # (the padding bits of the last byte are dropped at the end)
    legal = np.zeros(n, dtype=np.uint64)
    flips = np.zeros((64, n), dtype=np.uint64) if want_flips else None
    for cell in range(64):
        can = np.zeros_like(empty[cell])
        for step in DIRECTIONS:
            ray = _ray(cell, step)
            if len(ray) < 2:
                continue
            # run: the positions where `cell` is empty and every cell of the ray so far holds an opponent's stone
            run = empty[cell] & theirs[ray[0]]
            closed = []                                 # closed[k - 1]: ... and the mover's stone at ray[k] ends a run of k
            for k in range(1, len(ray)):
                closed.append(run & mine[ray[k]])
                run = run & theirs[ray[k]]
            turned = np.zeros_like(run)
            for j in range(len(closed) - 1, -1, -1):    # ray[j] is turned where the run closed after more than j stones
                turned = turned | closed[j]
                if want_flips:
                    flips[cell] |= np.unpackbits(turned, count=n).astype(np.uint64) << np.uint64(ray[j])
            can |= turned
        legal |= np.unpackbits(can, count=n).astype(np.uint64) << np.uint64(cell)
    if want_flips:
        # legal = empty and turns a stone, from the flips themselves
        from_flips = ((flips != 0).astype(np.uint64) << _CELLS[:, None]).sum(axis=0, dtype=np.uint64)
        assert np.array_equal(from_flips & ~(own | opp), legal) and np.array_equal(from_flips, legal)
        return legal, flips.T
    return legal


def reference(own, opp):
    """(legal, flips): legal (n,) uint64; flips (n, 64) uint64, flips[i, a] = the stones the mover of position i turns by
    playing cell a (0 where a is not empty or turns nothing)."""
    return _walk(own, opp, True)


def reference_legal(own, opp):
    """reference(own, opp)[0] without the flips (for batches of millions of boards)."""
    return _walk(own, opp, False)


@functools.lru_cache(maxsize=None)
def reference_of(noise_seed=None):
    """reference(*cases(noise_seed)[:2]), computed once."""
    own, opp, _ = cases(noise_seed)
    return _frozen(*reference(own, opp))


# ------------------------------------------------------------------------------------------------ shared helpers
def popcount(x):
    return np.unpackbits(np.ascontiguousarray(x, dtype=np.uint64).view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1).astype(np.int64)


def bits_of(mask):
    """(position, cell) of every set bit of a uint64 array: positions ascending, cells ascending within a position."""
    pos, cell = [], []
    for lo in range(0, len(mask), 65536):
        p, c = np.nonzero((mask[lo:lo + 65536, None] >> _CELLS) & _ONE)
        pos.append(p + lo)
        cell.append(c)
    return np.concatenate(pos).astype(np.int64), np.concatenate(cell).astype(np.int64)


def nth_bit(mask, r):
    """The cell of the r-th lowest set bit of every mask (r from 0); -1 where the mask is 0."""
    out = np.full(len(mask), -1, dtype=np.int64)
    for lo in range(0, len(mask), 65536):
        bit = ((mask[lo:lo + 65536, None] >> _CELLS) & _ONE).astype(bool)
        hit = bit & (np.cumsum(bit, axis=1) == np.asarray(r[lo:lo + 65536])[:, None] + 1)
        assert np.array_equal(hit.any(axis=1), mask[lo:lo + 65536] != 0)
        out[lo:lo + 65536] = np.where(hit.any(axis=1), hit.argmax(axis=1), -1)
    return out


def move_rows(own, opp, line_id, legal):
    """The rows (position, cell) the move kernels are asked: every EMPTY cell of the position's line, legal or not, and
    every legal move off it."""
    return bits_of((line_masks()[line_id] & ~(own | opp)) | legal)


def children(own, opp, flips, cell):
    """The boards after the mover plays `cell` turning `flips`, still from the mover's view: (own', opp')."""
    bit = _ONE << cell.astype(np.uint64)
    return own | flips | bit, opp & ~flips


def states_of(own, opp):
    """(n, 8, 8) float32 boards in the oracle's form: 1 = own, 2 = opp."""
    s = ((own[:, None] >> _CELLS) & _ONE).astype(np.float32) + 2 * ((opp[:, None] >> _CELLS) & _ONE).astype(np.float32)
    return np.ascontiguousarray(s.reshape(-1, 8, 8))


def boards_of(states):
    """states_of backwards: (own, opp) uint64 of (n, 8, 8) boards of 0 / 1 / 2."""
    s = np.asarray(states).reshape(-1, 64)
    return (((s == 1) * (_ONE << _CELLS)).sum(axis=1, dtype=np.uint64), ((s == 2) * (_ONE << _CELLS)).sum(axis=1, dtype=np.uint64))
