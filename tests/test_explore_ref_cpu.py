"""Exploring self-play without a GPU: the numpy reference of the draw (tests/explore_ref.py) on hand cases and on its
frequencies, and the ABI of the two entry points (include/iago_hip_serving.h: declared, exported, and refusing bad
arguments on the host with the entry point named)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import explore_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _row(**cells):
    n = np.zeros(64, np.int64)
    for k, v in cells.items():
        n[int(k[1:])] = v
    return n


# ---------------------------------------------------------------- the reference on hand cases
def test_a_single_legal_move_is_always_drawn():
    n = _row(c19=24)
    for w in (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF):
        assert explore_ref.draw_from_word(n, w) == 19
    for g in range(50):
        assert explore_ref.draw(n, seed=11, game_id=300 + g, turn=g % 8) == 19


def test_no_visits_falls_back_to_the_first_maximum():
    n = np.zeros(64, np.int64)
    assert explore_ref.draw_from_word(n, 0x12345678, legal=[44, 19, 26]) == 19   # every count 0: the lowest legal cell
    assert explore_ref.draw_from_word(n, 0x12345678) is None                     # (the row alone cannot say)


def test_the_extreme_words_pick_the_first_and_the_last_visited_move():
    n = _row(c19=1, c26=2, c37=0, c44=10)
    assert explore_ref.draw_from_word(n, 0) == 19
    assert explore_ref.draw_from_word(n, 0xFFFFFFFF) == 44
    n = _row(c5=0, c19=3, c26=7, c60=0)       # zero-visit cells at both ends
    assert explore_ref.draw_from_word(n, 0) == 19
    assert explore_ref.draw_from_word(n, 0xFFFFFFFF) == 26


def test_the_thresholds_are_the_integer_rule():
    """r = (w * N) >> 32 against the cumulative counts, at the words where r steps."""
    n = _row(c19=1, c26=2, c37=3, c44=10)     # N = 16: r = w >> 28
    for r, want in enumerate([19, 26, 26, 37, 37, 37] + [44] * 10):
        assert explore_ref.draw_from_word(n, r << 28) == want
        assert explore_ref.draw_from_word(n, ((r + 1) << 28) - 1) == want


def test_cells_without_visits_are_never_drawn():
    n = _row(c2=0, c19=5, c20=0, c26=1, c37=0, c44=3, c63=0)
    rng = np.random.RandomState(5)
    words = list(rng.randint(0, 2 ** 32, 4000, dtype=np.uint64)) + [0, 0xFFFFFFFF]
    seen = {explore_ref.draw_from_word(n, int(w)) for w in words}
    assert seen == {19, 26, 44}


def test_the_word_is_keyed_by_game_turn_and_the_explore_key():
    from oracle import oracle as orc
    seed = 0x0123456789ABCDEF
    assert explore_ref.EXPLORE_KEY == 0x4558504C == int.from_bytes(b"EXPL", "big")
    for g, t in ((0, 0), (300, 5), (2 ** 32 - 1, 7), (17, 11)):
        block = orc.philox(seed ^ (0x4558504C << 32), g, t >> 2, 0, 0)
        assert explore_ref.word(seed, g, t) == block[t & 3]
    # (a key of its own: not the rollouts' block, not a match's)
    assert explore_ref.word(seed, 3, 1) != orc.philox(seed, 3, 0, 0, 0)[1]
    assert explore_ref.word(seed, 3, 1) != orc.philox(seed ^ (0x4D415443 << 32), 3, 0, 0, 0)[1]
    assert explore_ref.word(seed, 2 ** 32 + 3, 1) == explore_ref.word(seed, 3, 1)   # (ids wrap at 32 bits)


# ---------------------------------------------------------------- frequencies
FREQ_SEED, FREQ_GAMES, FREQ_ROW = 2024, 65536, (1, 2, 3, 10)


def test_the_draws_follow_the_visit_counts():
    """Game ids 0 .. 65,535 at one turn under one seed: every move's count within 4.5 binomial sigma of
    N_games n[a] / N.  The draw is deterministic: this seed passes, and stays."""
    cells = (19, 26, 37, 44)
    n = np.zeros(64, np.int64)
    n[list(cells)] = FREQ_ROW
    total = int(n.sum())
    for turn in (0, 5):
        got = np.bincount([explore_ref.draw(n, FREQ_SEED, g, turn) for g in range(FREQ_GAMES)], minlength=64)
        assert got.sum() == FREQ_GAMES and not got[[a for a in range(64) if a not in cells]].any()
        for a in cells:
            p = n[a] / total
            sigma = np.sqrt(FREQ_GAMES * p * (1 - p))
            print("turn %d cell %d: %d draws, expected %.1f, sigma %.1f" % (turn, a, got[a], FREQ_GAMES * p, sigma))
            assert abs(got[a] - FREQ_GAMES * p) <= 4.5 * sigma, (turn, a, int(got[a]))


# ---------------------------------------------------------------- the ABI
def _lib():
    from iago_amd import _lib as L
    return L


def _error():
    return _lib().lib().iago_last_error().decode()


def test_the_serving_header_declares_and_the_library_exports_the_entry_points():
    L = _lib()
    text = open(os.path.join(ROOT, "include", "iago_hip_serving.h")).read()
    declared = set(re.findall(r"IAGO_API[^;(]*?\b(iago_\w+)\s*\(", text))
    for name in ("iago_mcts_search_explore", "iago_mcts_draw_move"):
        assert name in declared and name in L.SERVING_SYMBOLS and hasattr(L.lib(), name), name
        assert name not in open(os.path.join(ROOT, "include", "iago_hip.h")).read()
    assert "#define IAGO_EXPLORE_KEY 0x4558504Cu" in text
    assert L.EXPLORE_KEY == explore_ref.EXPLORE_KEY and L.EXPLORE_SEED_XOR == L.EXPLORE_KEY << 32
    assert L.EXPLORE_KEY != L.MATCH_KEY
    assert L.lib().iago_abi_version() == 13


def _explore_args(codes=(1, 1, 1, 1)):
    L = _lib()
    active = np.array(codes, np.uint8)
    tree = L.MctsTree()
    tree.n_games = len(codes)
    a = L.MctsSearchArgs()
    a.tree, a.active, a.max_turns = C.addressof(tree), active.ctypes.data, 128
    e = L.SearchExploreArgs()
    e.explore_turns = 8
    return a, e, (active, tree)


def test_search_explore_refusals():
    L = _lib()
    f = L.lib().iago_mcts_search_explore

    def refused(a, e, what):
        assert f(C.byref(a) if a is not None else None, C.byref(e) if e is not None else None, None) == -1
        assert _error().startswith("iago_mcts_search_explore") and what in _error(), _error()

    a, e, keep = _explore_args()
    refused(None, e, "null args")
    refused(a, None, "null args")
    for bad in (-1, 129):
        a, e, keep = _explore_args()
        e.explore_turns = bad
        refused(a, e, "explore_turns")
    a, e, keep = _explore_args()
    e.reserved0 = 1
    refused(a, e, "reserved")
    a, e, keep = _explore_args()
    e.reserved[2] = 5
    refused(a, e, "reserved")
    a, e, keep = _explore_args()
    a.max_turns = 0
    refused(a, e, "max_turns")
    for codes in ((1, 2, 1, 1), (3, 3, 3, 3), (0, 1, 1, 3)):
        a, e, keep = _explore_args(codes)
        refused(a, e, "match codes")
    # a hand-over in the same launch is checked as iago_mcts_search_park checks it
    out = [np.zeros(16, np.int32) for _ in range(3)]
    for field, value, what in (("park_empties", 21, "park_empties"), ("park_empties", -1, "park_empties"),
                               ("reserved0", 1, "reserved"), ("parked", None, "parked"),
                               ("streams", 0x1000, "streams")):
        a, e, keep = _explore_args()
        k = L.SearchParkArgs()
        k.park_empties = 8
        k.parked, k.stones, k.pass_flg = (b.ctypes.data for b in out)
        setattr(k, field, value)
        e.park = C.addressof(k)
        refused(a, e, what)
    # (everything above passed: the launch's own arguments are looked at next, by the search's common check)
    a, e, keep = _explore_args()
    assert f(C.byref(a), C.byref(e), None) == -1 and "null args" in _error()


def test_draw_move_refusals():
    L = _lib()
    f = L.lib().iago_mcts_draw_move
    buf = np.zeros(64, np.int64)
    nodes = np.zeros(64, np.int64)
    tree = L.MctsTree()
    tree.n_games, tree.capacity = 4, 8
    aligned = (nodes.ctypes.data + 31) & ~31
    tree.nodes = aligned
    tree.n_nodes = tree.root = tree.overflow = buf.ctypes.data
    p = buf.ctypes.data
    for args in ((None, None, 1, p, p, p, None, None),
                 (C.byref(tree), None, 1, None, p, p, None, None),
                 (C.byref(tree), None, 1, p, None, p, None, None),
                 (C.byref(tree), None, 1, p, p, None, None, None)):
        assert f(*args) == -1
        assert _error().startswith("iago_mcts_draw_move:"), _error()
    bad = L.MctsTree()
    bad.n_games, bad.capacity = 4, 0
    assert f(C.byref(bad), None, 1, p, p, p, None, None) == -1 and _error().startswith("iago_mcts_draw_move:")
    # no games: nothing to launch
    tree.n_games = 0
    assert f(C.byref(tree), None, 1, p, p, p, None, None) == 0


@pytest.mark.parametrize("bad", [True, -1, 8.0, "8", np.float32(3)])
def test_explore_turns_is_validated_before_the_device(bad):
    from iago_amd.engine import SelfPlayEngine

    class Stub(object):
        n_games = 4

        def __getattr__(self, name):
            raise AssertionError("explore_turns must be checked before the engine is touched (read %r)" % name)

    e = SelfPlayEngine(Stub())
    with pytest.raises(ValueError, match="explore_turns"):
        e.play(24, explore_turns=bad)
    with pytest.raises(ValueError, match="explore_turns"):
        e.play_stream(24, 8, explore_turns=bad)
    with pytest.raises(TypeError):
        e.play_match(24, explore_turns=8)     # matches do not explore
