"""The line cases (tests/line_cases.py) are complete, their plain reference is the C oracle's rules on every bare case and
on 8000 noisy ones, and the set holds the runs that matter: the longest run on every line in both directions, the same
run without its bracketing stone, and the run that reaches the edge."""
import numpy as np
import pytest

from oracle import oracle as orc

from . import line_cases as lc

NOISY_SAMPLE = 8000


@pytest.fixture(scope="module", params=sorted(lc.VARIANTS))
def variant(request):
    own, opp, line_id = lc.cases(lc.VARIANTS[request.param])
    legal, flips = lc.reference_of(lc.VARIANTS[request.param])
    return request.param, own, opp, line_id, legal, flips


def test_lines():
    lines = lc.all_lines()
    assert len(lines) == 38 and [len(l) for l in lines] == [8] * 16 + [3, 4, 5, 6, 7, 8, 7, 6, 5, 4, 3] * 2
    assert len({tuple(l) for l in lines}) == 38
    for l in lines:
        steps = {(b // 8 - a // 8, b % 8 - a % 8) for a, b in zip(l, l[1:])}
        assert len(steps) == 1 and steps <= {(0, 1), (1, 0), (1, 1), (1, -1)}, l
        # a whole line: its ends lie on the edge of the board
        (dr, dc), = steps
        for end, sign in ((l[0], -1), (l[-1], 1)):
            r, c = end // 8 + sign * dr, end % 8 + sign * dc
            assert not (0 <= r < 8 and 0 <= c < 8), l
    # every pair of cells a queen's move apart lies on exactly one line, except the corners' 2-cell diagonals
    on = sum(len(l) * (len(l) - 1) // 2 for l in lines)
    assert on == 16 * 28 + 2 * (28 + 2 * (3 + 6 + 10 + 15 + 21))


def test_counts_and_completeness():
    assert lc.N_CASES == 131166 == 16 * 6561 + 2 * 13095
    bare, noisy = lc.cases(None), lc.cases(lc.NOISE_SEED)
    lines, masks, first = lc.all_lines(), lc.line_masks(), lc.line_first()
    assert first[-1] == lc.N_CASES
    for own, opp, line_id in (bare, noisy):
        assert len(own) == len(opp) == len(line_id) == lc.N_CASES
        assert not (own & opp).any()
        assert np.array_equal(np.bincount(line_id), [3 ** len(l) for l in lines])
        assert np.all(np.diff(line_id) >= 0)
        for l, cells in enumerate(lines):
            lo, hi = first[l], first[l + 1]
            # the content code read back from the boards: every content once, in ascending order
            code = sum((((own[lo:hi] >> np.uint64(c)) & np.uint64(1)) + 2 * ((opp[lo:hi] >> np.uint64(c)) & np.uint64(1)))
                       .astype(np.int64) * 3 ** j for j, c in enumerate(cells))
            assert np.array_equal(code, np.arange(3 ** len(cells))), l
    on_line = masks[bare[2]]
    # both variants have the same line cells; the bare one has nothing else
    assert np.array_equal(bare[0], noisy[0] & on_line) and np.array_equal(bare[1], noisy[1] & on_line)
    assert np.array_equal(bare[2], noisy[2])
    assert not ((bare[0] | bare[1]) & ~on_line).any()
    # the noise: half of the cells off the line empty, the rest shared evenly
    off = lc.popcount(~on_line).sum()
    n_own, n_opp = lc.popcount(noisy[0] & ~on_line).sum(), lc.popcount(noisy[1] & ~on_line).sum()
    assert abs(n_own / off - 0.25) < 0.001 and abs(n_opp / off - 0.25) < 0.001     # (7.5M cells: sigma = 0.00016)
    # a second call returns the same arrays, and nobody can write to them
    assert lc.cases(lc.NOISE_SEED)[0] is noisy[0]
    with pytest.raises(ValueError):
        noisy[0][0] = 0


def _against_the_oracle(own, opp, legal, flips):
    """legal sets through orc.legal_actions, and the boards after orc.place_stone for every legal move."""
    states = lc.states_of(own, opp)
    got_legal = np.array([orc.actions_to_mask(orc.legal_actions(s, 1)) for s in states], dtype=np.uint64)
    bad = np.flatnonzero(got_legal != legal)
    assert len(bad) == 0, (int(bad[0]), hex(int(own[bad[0]])), hex(int(opp[bad[0]])))
    pos, cell = lc.bits_of(legal)
    after = states[pos].copy()
    for board, a in zip(after, cell.tolist()):
        orc.place_stone(board, a, 1)
    want_own, want_opp = lc.children(own[pos], opp[pos], flips[pos, cell], cell)
    got_own, got_opp = lc.boards_of(after)
    bad = np.flatnonzero((got_own != want_own) | (got_opp != want_opp))
    assert len(bad) == 0, (int(pos[bad[0]]), int(cell[bad[0]]))
    return len(pos)


def test_reference_is_the_oracle_on_every_bare_case():
    own, opp, _ = lc.cases(None)
    legal, flips = lc.reference_of(None)
    assert flips.shape == (lc.N_CASES, 64) and flips.dtype == np.uint64 and legal.dtype == np.uint64
    assert _against_the_oracle(own, opp, legal, flips) == 74512
    assert int((legal == 0).sum()) == 65286


def test_reference_is_the_oracle_on_a_noisy_sample():
    own, opp, _ = lc.cases(lc.NOISE_SEED)
    legal, flips = lc.reference_of(lc.NOISE_SEED)
    idx = (np.arange(NOISY_SAMPLE, dtype=np.int64) * lc.N_CASES) // NOISY_SAMPLE
    assert len(np.unique(idx)) == NOISY_SAMPLE
    moves = _against_the_oracle(own[idx], opp[idx], legal[idx], flips[idx])
    assert moves > 40000


def test_reference_legal_is_reference():
    own, opp, _ = lc.cases(lc.NOISE_SEED)
    legal, _ = lc.reference_of(lc.NOISE_SEED)
    assert np.array_equal(lc.reference_legal(own[::7], opp[::7]), legal[::7])
    # a batch that is no multiple of 8 positions (the bit vectors' last byte is partly padding)
    assert np.array_equal(lc.reference_legal(own[5:1008], opp[5:1008]), legal[5:1008])
    got = lc.reference(own[3:16], opp[3:16])
    assert np.array_equal(got[0], legal[3:16]) and np.array_equal(got[1], lc.reference_of(lc.NOISE_SEED)[1][3:16])


def test_flips_are_stones_of_the_opponent_in_line_with_the_move(variant):
    _, own, opp, _, legal, flips = variant
    assert not (flips & ~opp[:, None]).any()
    cells = np.uint64(1) << np.arange(64, dtype=np.uint64)
    occupied = ((own | opp)[:, None] & cells) != 0
    assert not flips[occupied].any()
    assert np.array_equal(((flips != 0) * cells).sum(axis=1, dtype=np.uint64), legal)


def test_helpers():
    mask = np.array([0, 1, 0x8000000000000001, 0x0000001008000000, 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)
    assert lc.popcount(mask).tolist() == [0, 1, 2, 2, 64]
    pos, cell = lc.bits_of(mask[:4])
    assert pos.tolist() == [1, 2, 2, 3, 3] and cell.tolist() == [0, 0, 63, 27, 36]
    assert lc.nth_bit(mask, np.array([0, 0, 1, 1, 40])).tolist() == [-1, 0, 63, 36, 40]
    own, opp = np.array([0x0000000810000000, 5], dtype=np.uint64), np.array([0x0000001008000000, 2], dtype=np.uint64)
    s = lc.states_of(own, opp)
    assert s.shape == (2, 8, 8) and s.dtype == np.float32 and np.array_equal(s[0], orc.initial_state())
    assert orc.state_to_bits(s[1]) == (5, 2)
    back = lc.boards_of(s)
    assert np.array_equal(back[0], own) and np.array_equal(back[1], opp)


def test_the_longest_runs_are_there(variant):
    """On every line, in both directions: the move that turns the longest run that fits (k - 2 stones on k cells), the
    same run with the bracketing stone missing, and the run that reaches the line's last cell."""
    name, own, opp, line_id, legal, flips = variant
    first, masks = lc.line_first(), lc.line_masks()
    for l, cells in enumerate(lc.all_lines()):
        k = len(cells)
        for way in (cells, cells[::-1]):
            run = sum(1 << c for c in way[1:-1])
            at = lambda states: first[l] + lc.code_of(states if way is cells else states[::-1])   # noqa: E731
            # (way[0] empty, way[1:-1] the opponent's, way[-1] as named)
            bracketed, open_end, to_the_edge = at([0] + [2] * (k - 2) + [1]), at([0] + [2] * (k - 2) + [0]), at([0] + [2] * (k - 1))
            for i in (bracketed, open_end, to_the_edge):
                assert line_id[i] == l and not ((own[i] | opp[i]) >> np.uint64(way[0])) & np.uint64(1)
                assert int(opp[i] & masks[l]) & run == run and not int(own[i] & masks[l]) & run
            # (the flips of way[0] in any other direction leave this line at once: `& masks[l]` is this direction's share)
            assert int(flips[bracketed, way[0]] & masks[l]) == run, (l, way)
            assert (int(legal[bracketed]) >> way[0]) & 1
            for i in (open_end, to_the_edge):
                assert int(flips[i, way[0]] & masks[l]) == 0, (l, way)
                if name == "bare":                                      # no stone of the mover's anywhere: no move at all
                    assert legal[i] == 0 and not flips[i].any()
            assert int(opp[to_the_edge] >> np.uint64(way[-1])) & 1 and not int((own | opp)[open_end] >> np.uint64(way[-1])) & 1
