"""The Value walk of two and four boards per workgroup on positions that load the board's edges, against the
one-board walk, bit for bit.

With two or more boards per workgroup a B tile of the walk's K loop is one row of a pair of boards, and the tiles
that lie wholly off the board -- row 0 under the taps of ky = 0, row 7 under those of ky = 2 -- are left out
(conv_trunk_body.hpp).  The one-board walk keeps quarter tiles and leaves nothing out.  A tile mapped to the
wrong cells, a zero slot that is not zero or a skipped tile that was not all zeros shows here: stones on rows 0
and 7, empty rows, full and empty boards, stones in the corners and the 8 symmetries of positions, in pairs whose
members differ, with the last pair of a batch ragged and full.
"""
import os

import numpy as np
import pytest
import torch

from tests.gpu_util import random_positions

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROW = lambda r: 0xFF << (8 * r)  # noqa: E731
COL = lambda c: 0x0101010101010101 << c  # noqa: E731
MASK = (1 << 64) - 1


def to_grid(b):
    return np.array([(b >> i) & 1 for i in range(64)], np.uint8).reshape(8, 8)


def to_bits(g):
    return sum(int(v) << i for i, v in enumerate(g.reshape(-1)))


def symmetries(own, opp):
    """The 8 images of a position under the board's rotations and reflections."""
    out = []
    go, gp = to_grid(own), to_grid(opp)
    for flip in (False, True):
        a, b = (go[:, ::-1], gp[:, ::-1]) if flip else (go, gp)
        for k in range(4):
            out.append((to_bits(np.rot90(a, k)), to_bits(np.rot90(b, k))))
    return out


def edge_positions():
    rng = np.random.default_rng(11)
    pos = [
        (0, 0),                                               # empty board
        (ROW(0), ROW(7)), (ROW(7), ROW(0)),                   # stones on rows 0 and 7 only
        (ROW(0) | ROW(7), 0), (0, ROW(0) | ROW(7)),
        (ROW(0), 0), (0, ROW(7)),
        (COL(0), COL(7)), (COL(0) | COL(7), ROW(0) | ROW(7) & ~(COL(0) | COL(7))),
        (0x5555555555555555, 0xAAAAAAAAAAAAAAAA),             # full boards
        (MASK, 0), (0, MASK),
        (MASK & ~ROW(3) & ~ROW(4), 0),                        # empty middle rows
        (0x8100000000000081, 0x4281000000008142),             # corners and their neighbours
        (0x0000000810000000, 0x0000001008000000),             # the start position
    ]
    for r in range(8):                                        # one full row at a time, other rows empty
        pos.append((ROW(r) & 0x5555555555555555, ROW(r) & 0xAAAAAAAAAAAAAAAA))
    for _ in range(6):                                        # random fillings of the two edge rows
        e = int(rng.integers(0, 1 << 16))
        f = int(rng.integers(0, 1 << 16)) & ~e
        lift = lambda v: (v & 0xFF) | ((v >> 8) << 56)     # noqa: E731
        pos.append((lift(e), lift(f)))
    own, opp = random_positions(6, seed=17)
    base = [(0x81000000000000C3, 0x7E0000000000003C)]  # edge rows, asymmetric
    base += [(int(o), int(p) & ~int(o)) for o, p in zip(own, opp)]
    for o, p in base:
        pos += symmetries(o, p)
    return [(o & MASK, p & MASK & ~o) for o, p in pos]


@pytest.fixture(scope="module")
def nets():
    from iago_amd import network, ops
    assert torch.cuda.is_available()
    torch.manual_seed(9)
    random_init = network.Value().cuda().eval()
    shipped = network.Value().load_npz(os.path.join(GOLDEN, "value_model.npz")).cuda().eval()
    return ops, {"random": random_init, "shipped": shipped}


def walk(value, bo, bp, count, boards, grid):
    out = torch.full((bo.shape[0],), -7.0, dtype=torch.float32, device="cuda")
    value.forward_boards_batch(bo, bp, torch.full((1,), count, dtype=torch.int32, device="cuda"), out, boards, grid)
    return out


@pytest.mark.parametrize("which", ["shipped", "random"])
@pytest.mark.parametrize("boards,grid", [(2, 256), (2, 5), (4, 256), (4, 3)])
def test_pair_walk_of_edge_positions_equals_one_board_walk(nets, which, boards, grid):
    ops, nn = nets
    value = nn[which]
    pos = edge_positions()
    n = len(pos)
    assert n % 2 == 1 and n % 4 != 0  # a ragged last pair and a ragged last four
    own = np.array([o for o, _ in pos], np.uint64)
    opp = np.array([p for _, p in pos], np.uint64)
    with torch.no_grad():
        for shift in (0, 1):  # every board once as the even and once as the odd member of its pair
            bo = ops.bits_to_tensor(np.roll(own, shift))
            bp = ops.bits_to_tensor(np.roll(opp, shift))
            want = walk(value, bo, bp, n, 1, 256)
            assert bool(torch.isfinite(want).all())
            for count in (n, n - 1, n - 2):  # the last pair ragged, full, ragged
                got = walk(value, bo, bp, count, boards, grid)
                assert torch.equal(got[:count], want[:count]), (which, boards, grid, shift, count)
                assert bool((got[count:] == -7.0).all())
    value.check_saturation()


@pytest.mark.parametrize("boards", [2, 4])
def test_symmetric_images_of_a_position_in_one_workgroup(nets, boards):
    """The 8 images of one position side by side: each pair's two boards are different images of it."""
    ops, nn = nets
    value = nn["shipped"]
    own, opp = random_positions(3, seed=23)
    pos = []
    for o, p in zip(own, opp):
        pos += symmetries(int(o), int(p) & ~int(o))
    bo = ops.bits_to_tensor(np.array([o for o, _ in pos], np.uint64))
    bp = ops.bits_to_tensor(np.array([p for _, p in pos], np.uint64))
    n = len(pos)
    with torch.no_grad():
        want = walk(value, bo, bp, n, 1, 256)
        got = walk(value, bo, bp, n, boards, 256)
    assert torch.equal(got, want)
    value.check_saturation()
