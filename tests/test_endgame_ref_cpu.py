"""The endgame references of tests/endgame_ref.py against each other and on hand-built positions, and the host side
of iago_solve_endgame (its header entry, its refusals before any device work).  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import oracle as orc

from . import endgame_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sq(r, c):
    return 1 << (8 * r + c)


def test_bitboard_twin_agrees_with_oracle_rules():
    own, opp = ref.late_positions(240, 3, 0, 8)
    kinds = set()
    for a, b in zip(own, opp):
        state = orc.bits_to_state(int(a), int(b))   # own = colour 1
        for wld in (False, True):
            want = ref.solve_state(state, 1, wld)
            assert ref.solve_bits(a, b, wld) == want, (hex(int(a)), hex(int(b)), wld)
        kinds.add(min(want[1], 0))
        assert ref.bit_legal(int(a), int(b)) == orc.actions_to_mask(orc.legal_actions(state, 1))
    assert 0 in kinds and -2 in kinds


def test_full_board():
    own = 0xFFFFFFFF00000000 | 0xFF
    opp = 0xFFFFFFFFFFFFFFFF & ~own
    assert ref.solve_bits(own, opp) == (40 - 24, -2)
    assert ref.solve_state(orc.bits_to_state(own, opp), 1) == (16, -2)
    assert ref.solve_bits(opp, own, wld=True) == (-1, -2)


def test_one_empty_only_one_side_can_take():
    # a0 empty; only colour 1 (own) brackets it (a1 opponent, a2 own); the opponent cannot take a0
    full = 0xFFFFFFFFFFFFFFFF
    opp = sq(1, 0)
    own = full & ~sq(0, 0) & ~opp
    assert ref.solve_bits(own, opp) == (64, 0)          # takes a0 and flips a1: 64 - 0
    # the side that cannot take it passes, the other one takes it
    score, move = ref.solve_bits(opp, own)
    assert (score, move) == (-64, -1)
    assert ref.solve_state(orc.bits_to_state(opp, own), 1) == (-64, -1)


def test_forced_pass_then_opponent_moves():
    # own: b1 alone; the opponent: c1..h1.  Own has no move (nothing to bracket), the opponent takes a1 over b1,
    # then nobody can move: 0 - 8 from own's view, after a pass
    own = sq(0, 1)
    opp = sum(sq(0, c) for c in range(2, 8))
    assert ref.bit_legal(own, opp) == 0 and ref.bit_legal(opp, own) == sq(0, 0)
    assert ref.solve_bits(own, opp) == (-8, -1)
    assert ref.solve_bits(opp, own) == (8, 0)
    assert ref.solve_state(orc.bits_to_state(own, opp), 1) == (-8, -1)
    assert ref.solve_bits(own, opp, wld=True) == (-1, -1)


def test_game_already_over():
    own, opp = sq(3, 3), sq(5, 5)       # nobody can move: 1 - 1 = 0, many empties
    assert ref.solve_bits(own, opp) == (0, -2)
    assert ref.solve_bits(own | sq(0, 0), opp) == (1, -2)
    assert ref.solve_bits(own | sq(0, 0), opp, wld=True) == (1, -2)


def test_tie_goes_to_the_lowest_index():
    # own at d1, e1 symmetric around the opponent run: two moves of equal value
    own = sq(0, 3)
    opp = sq(0, 2) | sq(0, 4)
    moves = ref.BitRules.moves((own, opp))
    assert moves == [1, 5]
    vals = [-ref.negamax(ref.BitRules, ref.BitRules.play((own, opp), m), -ref.INF, ref.INF, False) for m in moves]
    assert vals[0] == vals[1]
    assert ref.solve_bits(own, opp) == (vals[0], 1)
    assert ref.solve_state(orc.bits_to_state(own, opp), 1) == (vals[0], 1)


def test_serving_header_lists_the_solver():
    from iago_amd import _lib
    text = open(os.path.join(ROOT, "include", "iago_hip_serving.h")).read()
    assert sorted(set(re.findall(r"IAGO_API[^;(]*?\b(iago_\w+)\s*\(", text))) == sorted(_lib.SERVING_SYMBOLS)
    assert "iago_solve_endgame" in _lib.SERVING_SYMBOLS
    assert C.sizeof(_lib.EndgameArgs) == 8 * 3 + 4 * 4 + 8 * 5 + 8 * 4
    for name in ("IAGO_ENDGAME_EXACT 0", "IAGO_ENDGAME_WLD 1", "IAGO_ENDGAME_MAX_EMPTIES 20",
                 "IAGO_ENDGAME_MAX_TIME_MS 600000", "IAGO_ENDGAME_CTL_WORDS 4"):
        assert re.search(r"#define\s+" + name.replace(" ", r"\s+") + r"\b", text), name


def test_host_side_refusals():
    from iago_amd import _lib, build
    build.build()
    L = _lib.lib()
    buf = (C.c_uint64 * 8)()
    ctl = (C.c_uint32 * 4)()

    def args(**kw):
        a = _lib.EndgameArgs()
        for f in ("own", "opp", "score", "move", "nodes", "solved"):
            setattr(a, f, C.addressof(buf))
        a.ctl = C.addressof(ctl)
        a.n, a.mode, a.max_empties, a.time_limit_ms = 1, 0, 20, 1000
        for k, v in kw.items():
            if k == "reserved":
                a.reserved[1] = v
            else:
                setattr(a, k, v)
        return a

    assert L.iago_solve_endgame(None, None) == -1
    for kw in (dict(own=None), dict(opp=None), dict(score=None), dict(move=None), dict(nodes=None),
               dict(solved=None), dict(ctl=None), dict(n=-1), dict(mode=2), dict(mode=-1), dict(max_empties=21),
               dict(max_empties=-1), dict(time_limit_ms=0), dict(time_limit_ms=600001), dict(reserved0=1),
               dict(reserved=7)):
        assert L.iago_solve_endgame(C.byref(args(**kw)), None) == -1, kw   # IAGO_ERR_INVALID
        assert b"iago_solve_endgame" in L.iago_last_error()


def test_python_entry_points_refuse_bad_options():
    import torch
    from iago_amd import _lib, engine, ops
    t = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ValueError):
        ops.solve_endgame(t, t, mode="best")
    with pytest.raises(_lib.IagoError):
        ops.solve_endgame(t, t)                              # CPU tensors: no CPU fallback
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError):
            engine.solve_endgame(t, t, split_depth=bad)


# ------------------------------------------------------------------ the C reference (oracle/endgame_oracle.c)
def test_c_reference_equals_both_python_references():
    own, opp = ref.late_positions(520, 7, 0, 9)
    kinds, counts = set(), set()
    for a, b in zip(own, opp):
        state = orc.bits_to_state(int(a), int(b))
        for wld in (False, True):
            got = orc.solve_endgame(a, b, wld)[:2]
            assert got == ref.solve_bits(a, b, wld), (hex(int(a)), hex(int(b)), wld)
            assert got == ref.solve_state(state, 1, wld), (hex(int(a)), hex(int(b)), wld)
        kinds.add(min(got[1], 0))
        counts.add(ref.empties(a, b))
    assert kinds == {0, -1, -2} and counts == set(range(10))


def test_c_reference_on_the_hand_built_positions():
    full = 0xFFFFFFFFFFFFFFFF
    own = 0xFFFFFFFF00000000 | 0xFF
    assert orc.solve_endgame(own, full & ~own)[:2] == (16, -2)
    assert orc.solve_endgame(full & ~own, own, wld=True)[:2] == (-1, -2)
    opp = sq(1, 0)
    own = full & ~sq(0, 0) & ~opp
    assert orc.solve_endgame(own, opp)[:2] == (64, 0)
    assert orc.solve_endgame(opp, own)[:2] == (-64, -1)
    own, opp = sq(0, 1), sum(sq(0, c) for c in range(2, 8))
    assert orc.solve_endgame(own, opp)[:2] == (-8, -1)
    assert orc.solve_endgame(opp, own)[:2] == (8, 0)
    assert orc.solve_endgame(own, opp, wld=True)[:2] == (-1, -1)
    own, opp = sq(3, 3), sq(5, 5)
    assert orc.solve_endgame(own, opp)[:2] == (0, -2)
    assert orc.solve_endgame(own | sq(0, 0), opp)[:2] == (1, -2)
    assert orc.solve_endgame(own | sq(0, 0), opp, wld=True)[:2] == (1, -2)
    own, opp = sq(0, 3), sq(0, 2) | sq(0, 4)
    assert orc.root_values(own, opp) == {1: ref.solve_bits(own, opp)[0], 5: ref.solve_bits(own, opp)[0]}
    assert orc.solve_endgame(own, opp)[:2] == ref.solve_bits(own, opp) and orc.solve_endgame(own, opp)[1] == 1
    # a node budget that does not suffice is reported, not answered
    o, p = ref.late_positions(1, 9, 12, 12)
    assert orc.solve_endgame(o[0], p[0], limit=10) is None and orc.root_values(o[0], p[0], limit=10) is None


def test_c_root_values_equal_full_window_negamax():
    own, opp = ref.late_positions(120, 8, 1, 8)
    seen_tie = 0
    for a, b in zip(own, opp):
        a, b = int(a), int(b)
        for wld in (False, True):
            want = {m: -ref.negamax(ref.BitRules, ref.BitRules.play((a, b), m), -ref.INF, ref.INF, wld)
                    for m in ref.BitRules.moves((a, b))}
            got = orc.root_values(a, b, wld)
            assert got == want, (hex(a), hex(b), wld)
            if want:
                s, m, _ = orc.solve_endgame(a, b, wld)
                assert s == max(want.values()) and m == min(k for k, v in want.items() if v == s)
                seen_tie += sum(1 for v in want.values() if v == s) > 1
    assert seen_tie > 10


# ------------------------------------------------------------------ the committed fixture of deep positions
@pytest.fixture(scope="module")
def deep_fixture():
    from .conftest import load_json
    return load_json("endgame_deep.json")


def test_deep_fixture_families_and_row_counts(deep_fixture):
    from . import endgame_families as fam
    fam.check_fixture(deep_fixture)
    # "filled" says where the sparse boards make up for random games that are too heavy under the cap
    for e, f in deep_fixture["filled"].items():
        n = sum(1 for r in deep_fixture["rows"] if r["family"] == "sparse" and r["empties"] == int(e))
        assert n == f["sparse"] and n + min(f["random_exact"], f["random_wld"]) >= deep_fixture["rows_min"]


def test_deep_fixture_is_what_the_reference_computes(deep_fixture):
    """A seeded sample of the rows the reference solves fast (<= 300 k nodes), re-solved: identical, nodes included."""
    rows = [r for r in deep_fixture["rows"] if all(r[m] is None or max(r[m][2:]) <= 300000 for m in ("exact", "wld"))]
    assert len(rows) >= 100
    rs = np.random.RandomState(17)
    for i in rs.choice(len(rows), 120, replace=False):
        r = rows[i]
        for mode in ("exact", "wld"):
            if r[mode]:
                again = orc.solve_endgame(r["own"], r["opp"], mode == "wld")
                ordered = orc.solve_endgame(r["own"], r["opp"], mode == "wld", fastest_root=True)
                assert again[:2] == ordered[:2] and list(again) + [ordered[2]] == r[mode], (i, mode)
        if r["values"]:
            assert {str(m): v for m, v in orc.root_values(r["own"], r["opp"]).items()} == r["values"], i


def test_symmetry_helpers_are_the_boards_symmetries():
    from . import endgame_families as fam
    o, p = ref.late_positions(6, 19, 4, 7)
    for a, b in zip(o, p):
        vals = orc.root_values(a, b)
        for k in range(8):
            ta, tb = fam.sym_bits(k, a), fam.sym_bits(k, b)
            assert bin(ta).count("1") == bin(int(a)).count("1")
            assert orc.root_values(ta, tb) == {fam.sym_move(k, m): v for m, v in vals.items()}
    assert len({tuple(fam.sym_move(k, a) for a in range(64)) for k in range(8)}) == 8


def test_solve_endgame_raises_when_the_stack_word_is_set():
    """ops.solve_endgame's check of ctl (host side only: a faked ctl, no launch)."""
    import torch
    from iago_amd import _lib, ops
    out = dict(solved=torch.tensor([1, 0, 1], dtype=torch.uint8), ctl=torch.tensor([0, 3, 0, 0], dtype=torch.int32))
    ops._check_endgame_ctl(out, 3, 12, 1000)                      # a clean launch: nothing raised
    for ctl, what in (([0, 3, 0, 1], "stack"), ([1, 3, 0, 0], "gave up"), ([0, 3, 2, 0], "refused"),
                      ([1, 3, 1, 1], "stack")):
        out["ctl"] = torch.tensor(ctl, dtype=torch.int32)
        with pytest.raises(_lib.IagoError, match=what) as e:
            ops._check_endgame_ctl(out, 3, 12, 1000)
        assert e.value.result is out


# (family, entry point, phrases, limit, done flag) and what each fault says, word for word
LANE_FAMILIES = {
    "solver": dict(
        who="iago_solve_endgame", texts="_SOLVER_TEXTS", limit=12, done="solved",
        overflow="a position needed more stack frames than max_empties = 12 sizes (ctl[3] set): it was dropped with "
                 "solved = 0 and its outputs unwritten",
        job_overflow="a job needed more stack frames than max_empties = 12 sizes (ctl[3] set): it was dropped and its "
                     "root keeps solved = 0",
        gave_up="gave up at its clock limit (1000 ms): 1 of 3 positions unsolved",
        refused="2 positions refused (own & opp != 0, or more than max_empties = 12 empties)"),
    "yardstick": dict(
        who="iago_alphabeta_moves", texts="_ALPHABETA_TEXTS", limit=6, done="done",
        overflow="a position needed more stack frames than depth = 6 sizes (ctl[3] set)",
        job_overflow="a job needed more stack frames than depth = 6 sizes (ctl[3] set)",
        gave_up="gave up at its clock limit (1000 ms): 1 of 3 positions unfinished",
        refused="2 positions refused (own & opp != 0)"),
}


@pytest.mark.parametrize("family", sorted(LANE_FAMILIES))
def test_the_lane_searches_result_check_is_a_function_of_the_host_ctl_words(family):
    """ops._check_lane_ctl, what check_result runs for every entry point of both families, on CPU tensors and made-up
    ctl words: a clean launch, a give-up, refusals, a stack overflow and -- a split launch -- a job overflow, which comes
    first and carries the 64-bit count of ctl[4] / [5] as jobs_needed.  The texts are the entry points' own."""
    import torch
    from iago_amd import _lib, ops
    f = LANE_FAMILIES[family]
    out = {f["done"]: torch.tensor([1, 0, 1], dtype=torch.uint8)}

    def run(who, ctl, job_capacity=None):
        ops._check_lane_ctl(who, out, ctl, getattr(ops, f["texts"]), f["limit"], 1000, 3, f["done"], job_capacity)

    def raised(who, ctl, job_capacity=None):
        with pytest.raises(_lib.IagoError) as e:
            run(who, ctl, job_capacity)
        assert e.value.result is out
        return e.value

    who, split = f["who"], f["who"] + "_split"
    run(who, [0, 3, 0, 0])                                        # clean launches: nothing raised
    run(split, [0, 9, 0, 0, 9, 0, 0, 0], 9)
    run(split, [0, 0, 0, 0, 0, 0, 0, 0], 0)
    for name, ctl, cap, key in ((who, [1, 3, 0, 0], None, "gave_up"), (who, [0, 3, 2, 0], None, "refused"),
                                (who, [0, 3, 0, 1], None, "overflow"), (who, [1, 3, 2, 1], None, "overflow"),
                                (who, [1, 3, 2, 0], None, "gave_up"),
                                (split, [1, 9, 0, 0, 9, 0, 0, 0], 9, "gave_up"),
                                (split, [0, 9, 2, 0, 9, 0, 0, 0], 9, "refused"),
                                (split, [0, 9, 0, 1, 9, 0, 0, 0], 9, "job_overflow"),
                                (split, [1, 9, 2, 1, 9, 0, 0, 0], 9, "job_overflow")):
        err = raised(name, ctl, cap)
        assert str(err) == "%s: %s" % (name, f[key]), (name, ctl)
        assert not hasattr(err, "jobs_needed")
    # the jobs did not fit: first of all, with the count needed (ctl is read back as int32: a negative low word)
    for ctl, needed in (([0, 0, 0, 0, 10, 0, 1, 0], 10), ([1, 0, 2, 1, 10, 0, 1, 0], 10),
                        ([0, 0, 0, 0, -1, 2, 1, 0], 3 * 2 ** 32 - 1)):
        err = raised(split, ctl, 9)
        assert str(err) == "%s: the search needs %d jobs, job_capacity holds 9: nothing was searched" % (split, needed)
        assert err.jobs_needed == needed
