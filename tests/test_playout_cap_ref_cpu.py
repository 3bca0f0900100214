"""Playout-cap randomisation on the CPU: the reference rule (tests/playout_cap_ref.py) has a key of its own, its two
ends, and the frequency it promises; the oracle's search leaves children after N_FAST playouts from the opening (the GPU
tests' fast budget); the entry points are declared, exported and refuse bad arguments without a device."""
import math
import os
import re

import numpy as np

from oracle import mcts_py
from oracle import oracle as orc
from tests import explore_ref, playout_cap_ref as cap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 11


def test_the_cap_word_is_not_the_explore_word():
    same = 0
    for g in range(64):
        for t in range(8):
            same += cap.word(SEED, 300 + g, t) == explore_ref.word(SEED, 300 + g, t)
    assert same == 0
    assert cap.CAP_KEY not in (explore_ref.EXPLORE_KEY, 0x4D415443, 0x52504C59)   # (the draw's, a match's, the replay's)


def test_256_makes_every_turn_full():
    assert all(cap.is_full(SEED, g, t, 256) for g in range(0, 4096, 37) for t in range(128))
    assert all(cap.valid_code(SEED, g, t, 256) == 1 for g in range(8) for t in range(8))
    assert cap.budget(SEED, 5, 3, 256, 32, 18) == 32


def test_a_quarter_of_the_turns_are_full_at_64():
    n, p = 4096 * 8, 64 / 256
    full = sum(cap.is_full(SEED, g, t, 64) for g in range(4096) for t in range(8))
    bound = 5 * math.sqrt(n * p * (1 - p))          # 5 binomial standard deviations: 391.9
    assert int(bound) + 1 == 392
    print("full turns: %d of %d (a quarter: %d, bound %d)" % (full, n, n // 4, 392))
    assert abs(full - n * p) <= 392


def test_eighteen_playouts_from_the_opening_leave_children():
    """n_thr = 15: a fresh root expands at its 16th playout, so N_FAST = 18 leaves the root three visited playouts'
    worth of children (and 15 would leave none: the engine's ValueError)."""
    def search(n):
        m = mcts_py.MCTS(lambda x: np.full(64, 1 / 64, np.float32), lambda x: np.float32(0.0), lambda s, c: 0,
                         lmbda=0.5, c_puct=1.0, n_thr=15)
        m.get_move(orc.initial_state(), 1, n)
        return m.root.children
    kids = search(18)
    assert len(kids) == 4 and sum(ch.n_visits for ch in kids.values()) == 3
    assert len(search(15)) == 0


def test_entry_points_are_declared_exported_and_refuse():
    import ctypes as C
    from iago_amd import _lib as L, build
    build.build()
    text = open(os.path.join(ROOT, "include", "iago_hip_serving.h")).read()
    declared = set(re.findall(r"IAGO_API[^;(]*?\b(iago_\w+)\s*\(", text))
    for name in ("iago_mcts_search_cap", "iago_mcts_cap_mask"):
        assert name in declared and name in L.SERVING_SYMBOLS and hasattr(L.lib(), name), name
    assert re.search(r"#define\s+IAGO_CAP_KEY\s+0x43415050u", text) and L.CAP_KEY == cap.CAP_KEY
    assert "iago_search_cap_args" in text
    assert [f[0] for f in L.SearchCapArgs._fields_] == ["n_fast", "full_per_256", "explore_turns", "reserved0", "streams",
                                                        "park", "reserved"]
    assert C.sizeof(L.SearchCapArgs) == 64
    lib = L.lib()
    assert lib.iago_mcts_search_cap(None, None, None) == L.IAGO_ERR_INVALID
    assert lib.iago_last_error().startswith(b"iago_mcts_search_cap")
    a, c = L.MctsSearchArgs(), L.SearchCapArgs()
    assert lib.iago_mcts_search_cap(C.byref(a), None, None) == L.IAGO_ERR_INVALID
    a.n_sims = 32
    for n_fast, full, e, r0, r3 in ((0, 64, 0, 0, 0), (33, 64, 0, 0, 0), (18, 0, 0, 0, 0), (18, 257, 0, 0, 0),
                                    (18, 64, -1, 0, 0), (18, 64, 129, 0, 0), (18, 64, 0, 1, 0), (18, 64, 0, 0, 1),
                                    (18, 64, 0, 0, 0)):     # (the last: max_turns == 0)
        c = L.SearchCapArgs()
        c.n_fast, c.full_per_256, c.explore_turns, c.reserved0 = n_fast, full, e, r0
        c.reserved[3] = r3
        assert lib.iago_mcts_search_cap(C.byref(a), C.byref(c), None) == L.IAGO_ERR_INVALID, (n_fast, full, e, r0, r3)
        assert lib.iago_last_error().startswith(b"iago_mcts_search_cap")
    c = L.SearchCapArgs()
    c.n_fast, c.full_per_256 = 18, 64
    k = L.SearchParkArgs()                                  # (a bad park: no outputs)
    c.park = C.addressof(k)
    assert lib.iago_mcts_search_cap(C.byref(a), C.byref(c), None) == L.IAGO_ERR_INVALID
    assert b"park" in lib.iago_last_error()
    for full in (0, 257):
        assert lib.iago_mcts_cap_mask(SEED, None, None, full, 0, None, None) == L.IAGO_ERR_INVALID
    assert lib.iago_mcts_cap_mask(SEED, None, None, 64, 4, None, None) == L.IAGO_ERR_INVALID
    assert lib.iago_mcts_cap_mask(SEED, None, None, 64, 0, None, None) == L.IAGO_OK


def test_playout_cap_arg():
    import pytest
    from iago_amd import ops
    assert ops.playout_cap_arg(None, 32) is None
    assert ops.playout_cap_arg((18, 64), 32) == (18, 64) and ops.playout_cap_arg([32, 256], 32) == (32, 256)
    for bad in ((0, 64), (33, 64), (18, 0), (18, 257), (18,), 18, (18.0, 64), (True, 64), "ab", (18, 64, 1)):
        with pytest.raises(ValueError, match="playout_cap"):
            ops.playout_cap_arg(bad, 32)
