"""iago_solve_endgame against an independent reference up to 20 empties: the rows of tests/golden/endgame_deep.json
(positions and their results by the C reference oracle/endgame_oracle.c, made by tests/golden/make_endgame_golden.py)
through ops.solve_endgame / engine.solve_endgame.  Every launch runs under an explicit clock of 4 x the time the
fixture's node cap implies at the measured rate of the deepest lane of such a launch (0.4 M nodes/s in a wave shared
with other deep positions, LABNOTES "Endgame against the C reference": 2 M nodes -> 5 s -> 20 s), every test asserts
that all positions were solved, that the launch neither gave up (ctl[0]) nor ran out of stack (ctl[3]) and refused
(ctl[2]) only what the test means to be refused, and no fixture row of a mode is left out."""
import time

import numpy as np
import pytest

from iago_amd import _lib, engine, ops

from . import endgame_families as fam
from . import endgame_ref as ref
from .conftest import load_json

pytestmark = pytest.mark.gpu

LANE_NODES_PER_S = 0.4e6   # LABNOTES "Endgame against the C reference"
MODES = ("exact", "wld")


@pytest.fixture(scope="module")
def fx():
    return load_json("endgame_deep.json")


def _limit_ms(fx):
    return int(4 * 1000 * fx["n_cap"] / LANE_NODES_PER_S)


def _arrays(rows):
    return np.array([r["own"] for r in rows], np.uint64), np.array([r["opp"] for r in rows], np.uint64)


def _solve(own, opp, mode, limit_ms, refused=0, **kw):
    """One launch; the assertions every test makes."""
    t0 = time.time()
    r = ops.solve_endgame(ops.bits_to_tensor(own), ops.bits_to_tensor(opp), mode=mode, time_limit_ms=limit_ms,
                          check_result=False, **kw)
    r = {k: v.cpu().numpy() for k, v in r.items()}
    r["seconds"] = time.time() - t0
    assert r["ctl"][0] == 0, "gave up"
    assert r["ctl"][3] == 0, "out of stack"
    assert r["ctl"][2] == refused
    if not refused:
        assert r["solved"].all()
    return r


def _assert_rows(r, rows, mode, what=""):
    for i, row in enumerate(rows):
        assert r["solved"][i] == 1, (what, i)
        assert (int(r["score"][i]), int(r["move"][i])) == tuple(row[mode][:2]), (what, mode, i, row["family"],
                                                                                  hex(row["own"]), hex(row["opp"]))


# ------------------------------------------------------------------ a. 11 .. 20 empties, row for row
@pytest.mark.parametrize("mode", MODES)
def test_every_fixture_row(fx, mode):
    rows = [r for r in fx["rows"] if r[mode]]
    assert len(rows) == sum(1 for r in fx["rows"] if r[mode])
    for e in range(11, 21):
        assert sum(1 for r in rows if r["empties"] == e) >= 8, e
    own, opp = _arrays(rows)
    r = _solve(own, opp, mode, _limit_ms(fx))
    # the kernel's node count next to the reference's, and the lane rate of the deepest row
    ratio = [r["nodes"][i] / max(row[mode][3], 1) for i, row in enumerate(rows) if row[mode][3] >= 1000]
    plain = [r["nodes"][i] / max(row[mode][2], 1) for i, row in enumerate(rows) if row[mode][2] >= 1000]
    print("\n[endgame %s] rows %d, launch %.2f s, max kernel nodes %d (reference, root ordered alike: %d), "
          "kernel/reference nodes: median %.3f max %.3f (root in ascending index: median %.2f max %.2f), deepest lane "
          ">= %.2f M nodes/s" % (
              mode, len(rows), r["seconds"], r["nodes"].max(), max(row[mode][3] for row in rows),
              float(np.median(ratio)), max(ratio), float(np.median(plain)), max(plain),
              r["nodes"].max() / r["seconds"] / 1e6))
    _assert_rows(r, rows, mode)
    # once more per empties count as engine.solve_endgame launches it: max_empties = the batch's largest count, so
    # another number of stack levels and another layout of the frames in LDS -- same score, move and nodes
    for e in sorted({row["empties"] for row in rows}):
        sel = [i for i, row in enumerate(rows) if row["empties"] == e]
        assert engine._most_empties(ops.bits_to_tensor(own[sel]), ops.bits_to_tensor(opp[sel])) == e
        part = engine.solve_endgame(ops.bits_to_tensor(own[sel]), ops.bits_to_tensor(opp[sel]), mode=mode,
                                    time_limit_ms=_limit_ms(fx))
        part = {k: v.cpu().numpy() for k, v in part.items()}
        assert part["solved"].all() and not part["ctl"][0] and not part["ctl"][2] and not part["ctl"][3]
        for k in ("score", "move", "nodes"):
            assert (part[k] == r[k][sel]).all(), (k, e)


# ------------------------------------------------------------------ b. the adversarial families
@pytest.mark.parametrize("family", [f for f in fam.FAMILIES if f not in ("random", "sym")])
def test_family(fx, family):
    rows = [r for r in fx["rows"] if r["family"] == family]
    assert rows
    for mode in MODES:
        sel = [r for r in rows if r[mode]]
        assert len(sel) == len(rows) or family == "sparse"
        own, opp = _arrays(sel)
        _assert_rows(_solve(own, opp, mode, _limit_ms(fx)), sel, mode, family)
    if family == "ties":   # the rule stated without either solver's move order
        own, opp = _arrays(rows)
        r = _solve(own, opp, "exact", _limit_ms(fx))
        w = _solve(own, opp, "wld", _limit_ms(fx))
        for i, row in enumerate(rows):
            vals = {int(m): v for m, v in row["values"].items()}
            assert int(r["score"][i]) == max(vals.values())
            assert int(r["move"][i]) == min(m for m, v in vals.items() if v == max(vals.values()))
            sign = {m: (v > 0) - (v < 0) for m, v in vals.items()}
            assert int(w["move"][i]) == min(m for m, s in sign.items() if s == max(sign.values()))
    if family in ("over", "rootpass"):
        want = -2 if family == "over" else -1
        r = _solve(*_arrays(rows), "exact", _limit_ms(fx))
        assert all(int(m) == want or row["empties"] <= 1 for m, row in zip(r["move"], rows))


@pytest.mark.parametrize("mode", MODES)
def test_symmetries(fx, mode):
    rows = [r for r in fx["rows"] if r["family"] == "sym"]
    assert len(rows) >= 64
    own = np.array([fam.sym_bits(k, r["own"]) for r in rows for k in range(8)], np.uint64)
    opp = np.array([fam.sym_bits(k, r["opp"]) for r in rows for k in range(8)], np.uint64)
    res = _solve(own, opp, mode, _limit_ms(fx))
    for i, row in enumerate(rows):
        vals = {int(m): (v if mode == "exact" else (v > 0) - (v < 0)) for m, v in row["values"].items()}
        best = [m for m, v in vals.items() if v == max(vals.values())]
        for k in range(8):
            j = 8 * i + k
            assert int(res["score"][j]) == row[mode][0] == max(vals.values()), (i, k)
            assert int(res["move"][j]) == min(fam.sym_move(k, m) for m in best), (i, k)


# ------------------------------------------------------------------ c. the stack rule at every size
def _batch_for(fx, k, mode, n=16):
    """(own, opp, expected (score, move)) of positions with exactly k empties plus a few with fewer: from the fixture
    (k >= 11, the lightest rows of the count) or solved by endgame_ref.solve_bits."""
    own, opp, want = np.zeros(0, np.uint64), np.zeros(0, np.uint64), []
    if k >= 11:
        rows = sorted((r for r in fx["rows"] if r["empties"] == k and r[mode]), key=lambda r: r[mode][3])[:n]
        rows += [r for r in fx["rows"] if 11 <= r["empties"] < k and r[mode] and r[mode][3] < 100000][:4]
        own, opp = _arrays(rows)
        want = [tuple(r[mode][:2]) for r in rows]
    else:
        own, opp = ref.late_positions(n if k <= 8 else 6, 300 + k, k, k)
    if k > 0:   # fewer empties than max_empties admits, at every k
        o2, p2 = ref.late_positions(4, 400 + k, 0, min(k - 1, 8))
        own, opp = np.concatenate([own, o2]), np.concatenate([opp, p2])
    want += [ref.solve_bits(a, b, wld=mode == "wld") for a, b in zip(own[len(want):], opp[len(want):])]
    return own, opp, want


@pytest.mark.parametrize("k", range(21))
def test_stack_rule_at_max_empties(fx, k):
    for mode in MODES:
        own, opp, want = _batch_for(fx, k, mode)
        assert len(own) >= 6 and max(ref.empties(a, b) for a, b in zip(own, opp)) == k
        r = _solve(own, opp, mode, _limit_ms(fx), max_empties=k)
        assert [(int(s), int(m)) for s, m in zip(r["score"], r["move"])] == want, (k, mode)
        # one position with k + 1 empties in the same wave: refused, its neighbours still solved
        xo, xp = ref.late_positions(1, 500 + k, k + 1, k + 1)
        at = len(own) // 2
        own2, opp2 = np.insert(own, at, xo[0]), np.insert(opp, at, xp[0])
        r = _solve(own2, opp2, mode, _limit_ms(fx), refused=1, max_empties=k)
        assert r["solved"][at] == 0 and r["solved"].sum() == len(own)
        got = [(int(s), int(m)) for i, (s, m) in enumerate(zip(r["score"], r["move"])) if i != at]
        assert got == want, (k, mode)
        if mode == "wld":   # and what a caller who checks the result sees
            with pytest.raises(_lib.IagoError, match="refused"):
                ops.solve_endgame(ops.bits_to_tensor(own2), ops.bits_to_tensor(opp2), mode=mode, max_empties=k,
                                  time_limit_ms=_limit_ms(fx))


@pytest.mark.parametrize("k", [17])
def test_stack_rule_odd_batches(fx, k):
    own, opp, want = _batch_for(fx, k, "exact", n=8)
    reps = np.arange(64 * 3 + 7) % len(own)
    r = _solve(own[reps], opp[reps], "exact", _limit_ms(fx), max_empties=k)
    assert [(int(s), int(m)) for s, m in zip(r["score"], r["move"])] == [want[i] for i in reps]
    one = _solve(own[:1], opp[:1], "exact", _limit_ms(fx), max_empties=k)
    assert (int(one["score"][0]), int(one["move"][0])) == want[0] and one["nodes"][0] == r["nodes"][0]


# ------------------------------------------------------------------ d. the root split as it is used
def _split(own, opp, mode, depth, limit_ms):
    r = engine.solve_endgame(ops.bits_to_tensor(own), ops.bits_to_tensor(opp), mode=mode, split_depth=depth,
                             time_limit_ms=limit_ms)
    r = {k: v.cpu().numpy() for k, v in r.items()}
    # (the split's `solved` is all ones by construction: what guards the leaves is ops.solve_endgame's check of ctl,
    # which raises inside engine.solve_endgame; ctl is the leaf launch's own)
    assert r["solved"].all() and r["ctl"][0] == 0 and r["ctl"][2] == 0 and r["ctl"][3] == 0
    return r


def test_split_depth_4_at_9_and_10_empties(fx):
    own, opp = ref.late_positions(12, 601, 9, 10)
    for mode in MODES:
        r = _split(own, opp, mode, 4, _limit_ms(fx))
        for i, (a, b) in enumerate(zip(own, opp)):
            assert (int(r["score"][i]), int(r["move"][i])) == ref.solve_bits(a, b, wld=mode == "wld"), (mode, i)


def _leaves(own, opp, depth):
    """The number of leaves engine.solve_endgame's split of `depth` plies hands to the kernel."""
    level, n = [(int(own), int(opp))], 0
    for _ in range(depth):
        nxt = []
        for a, b in level:
            ms = ref.BitRules.moves((a, b))
            if ms:
                nxt += [ref.BitRules.play((a, b), m) for m in ms]
            elif ref.bit_legal(b, a):
                nxt.append((b, a))
            else:
                n += 1
        level = nxt
    return n + len(level)


@pytest.mark.parametrize("depth", [1, 2, 3, 4])
def test_split_against_the_fixture(fx, depth):
    # the three lightest rows of every count (the split solves its leaves with full windows: more nodes in all than
    # the plain launch, so the heaviest rows would take a launch each) and six rows of each pass / early-end family
    both = [r for r in fx["rows"] if r["exact"] and r["wld"]]
    rows = []
    for e in range(12, 17):
        rows += sorted((r for r in both if r["family"] in ("random", "sym") and r["empties"] == e),
                       key=lambda r: r["exact"][3])[:3]
    plain = len(rows)
    assert plain == 15 and [r["empties"] for r in rows] == [e for e in range(12, 17) for _ in range(3)]
    for f in ("pass2", "rootpass", "passend", "over", "over1"):
        rows += [r for r in both if r["family"] == f][:6]
    assert {r["family"] for r in rows} >= {"pass2", "rootpass", "passend", "over", "over1"}
    own, opp = _arrays(rows)
    for mode in MODES:
        mixed = _split(own, opp, mode, depth, _limit_ms(fx))          # one mixed batch
        _assert_rows(mixed, rows, mode, "split %d" % depth)
        for i in list(range(0, plain, 4)) + list(range(plain, len(rows), 5)):   # and position by position
            one = _split(own[i:i + 1], opp[i:i + 1], mode, depth, _limit_ms(fx))
            _assert_rows(one, rows[i:i + 1], mode, "split %d row %d" % (depth, i))
            assert one["nodes"][0] >= _leaves(own[i], opp[i], depth)
            assert one["nodes"][0] == mixed["nodes"][i]
