#!/usr/bin/env python3
"""Deep endgame positions with their exact results, solved by the C reference (oracle/endgame_oracle.c):

    python tests/golden/make_endgame_golden.py      -> tests/golden/endgame_deep.json

Deterministic (seeded; the thread pool only changes who solves what).  Data only.  The fixture holds the position
families that tests/test_endgame_deep_gpu.py runs iago_solve_endgame on and that tests/test_endgame_ref_cpu.py checks
for their properties (tests/endgame_families.py has the property checks, shared by this script and the tests):

  random     seeded uniform-random games (endgame_ref.late_positions), 11 .. 20 empties
  sparse     17 .. 20 empties, one side with at most 8 stones: most empties can never be played, the trees are small
             at full stack depth.  Also fills an empties count up to ROWS_MIN rows per mode where random games under
             the node cap are too rare (see "filled" in the fixture)
  pass2      the principal line has >= 2 forced passes at different plies
  rootpass   the side to move must pass (move -1) and the opponent has >= 2 replies tied for its best
  passend    a pass of the principal line is followed by one move and the end of the game
  over       the game is over at the root (move -2) with >= 8 empties: wipe-outs and sealed-off boards; and full
             boards / last-square positions with the scores +64, -64, 0
  over1      a root move ends the game one ply below the root with >= 8 empties left
  ties       >= 3 root moves share the best exact value and the lowest of them is NOT the move a fewest-replies-first
             order tries first
  sym        base positions of 12 .. 16 empties with the exact value of every root move (the tests apply the 8 board
             symmetries themselves)

A row: family, own, opp (own = the side to move, bit a = row * 8 + col), empties, exact = [score, move, nodes,
nodes_k] or null, wld = [sign, move, nodes, nodes_k] or null, values = {move: exact value} (ties, sym) or null.  nodes
is the reference's count with its root in ascending index, nodes_k its count with the root ordered fewest-replies-first
like the kernel's (the same answer from another tree; on the rows of this fixture the kernel's own count is within
0.6 % of nodes_k, while it runs up to 1.7 times (exact) and 23 times (wld) above the ascending-index count).
A mode is null where either count is
above N_CAP: the row is then not used in that mode.

N_CAP: the deepest position of a launch should take about 5 s.  A lane alone in its wave runs ~0.8 M nodes/s
(LABNOTES "Exact endgame"); the deepest lane of a launch of these rows, sharing its wave with 12 - 40 other deep
positions, ran 0.39 - 0.54 M nodes/s (LABNOTES "Endgame against the C reference"): 0.4 M nodes/s x 5 s = 2 M nodes.

Measured with the C reference on one CPU core (4 - 5 M nodes/s), no node limit, mean seconds and nodes per position
of endgame_ref.late_positions (6 positions at 12 - 16 empties, 4 at 18 and 20; the largest of them in brackets):

  empties   exact s       exact nodes                  wld s     wld nodes
       12     0.012            58,278                  0.002         9,696
       14     0.131           655,216                  0.014        70,600
       16     1.187         6,018,867 (19.3 M)         0.055       280,133 (1.5 M)
       18       3.2        12,238,176 (21.8 M)           0.2       938,327 (3.5 M)
       20      58.4       274,488,353 (509 M, 107 s)    13.4    53,301,598 (146 M, 36 s)

So from 17 empties on the script solves a position of a random game under the cap only (one that needs more costs
the cap, 0.4 s per mode and root order): of 64 candidates per count 12 stay under it in WLD at every count, in exact
mode 6 at 17 empties and none above; there the sparse boards supply the rows ("filled" in the fixture counts both).
The whole script takes 2 - 3 minutes with 8 worker threads (it starts 16 at the most); the CPU test that re-solves a
sample of the rows of at most 300 k nodes takes under 25 s.
"""
import json
import os
import sys
import time
from multiprocessing.pool import ThreadPool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import oracle as orc  # noqa: E402
from tests import endgame_families as fam  # noqa: E402
from tests import endgame_ref as ref  # noqa: E402

N_CAP = 2000000
ROWS_MIN = 8
ROWS_RANDOM = 12
FULL = ref.FULL


def one_mode(own, opp, wld):
    """[score, move, nodes, nodes with the root ordered like the kernel's] or None when either count is above N_CAP."""
    r = orc.solve_endgame(own, opp, wld, N_CAP)
    k = r and orc.solve_endgame(own, opp, wld, N_CAP, fastest_root=True)
    if not k:
        return None
    assert r[:2] == k[:2]
    return list(r) + [k[2]]


def solve_row(family, own, opp, values=False):
    """A fixture row, or None when neither mode stays under N_CAP."""
    own, opp = int(own), int(opp)
    ex, wl = one_mode(own, opp, False), one_mode(own, opp, True)
    if ex is None and wl is None:
        return None
    vals = None
    if values:
        vals = orc.root_values(own, opp, False, N_CAP)
        if vals is None or ex is None:
            return None
        vals = {str(m): v for m, v in sorted(vals.items())}
    return dict(family=family, own=own, opp=opp, empties=ref.empties(own, opp),
                exact=ex, wld=wl, values=vals)


def both_modes(family, own, opp, keep):
    """A row solved in both modes that `keep` accepts, or None."""
    r = solve_row(family, own, opp)
    return r if r and r["exact"] and r["wld"] and keep(r) else None


def sparse_board(rs, e, few):
    """e empties, the rest own but for at most `few` opponent stones (or the other way round)."""
    cells = rs.permutation(64)
    empty = sum(1 << int(c) for c in cells[:e])
    k = int(rs.randint(1, few + 1))
    minority = sum(1 << int(c) for c in cells[e:e + k])
    majority = FULL & ~empty & ~minority
    return (majority, minority) if rs.randint(2) else (minority, majority)


def main():
    t_start = time.time()
    pool = ThreadPool(min(16, os.cpu_count() or 1))
    rows, filled = [], {}

    # ---- random games, 11 .. 20 empties
    timing = {}
    for e in range(11, 21):
        own, opp = ref.late_positions(24 if e <= 16 else 64, 1000 + e, e, e)
        t0 = time.time()
        got = pool.map(lambda ab: solve_row("random", ab[0], ab[1]), list(zip(own, opp)))
        timing[e] = (time.time() - t0, len(own))
        n_ex = n_wl = 0
        for r in got:
            if r is None:
                continue
            keep_ex, keep_wl = r["exact"] is not None and n_ex < ROWS_RANDOM, r["wld"] is not None and n_wl < ROWS_RANDOM
            if not (keep_ex or keep_wl):
                continue
            r = dict(r, exact=r["exact"] if keep_ex else None, wld=r["wld"] if keep_wl else None)
            n_ex, n_wl = n_ex + keep_ex, n_wl + keep_wl
            rows.append(r)

    # ---- sparse boards, 17 .. 20 empties (and the fill-up of thin counts)
    rs = np.random.RandomState(77)
    for e in range(17, 21):
        cands = [sparse_board(rs, e, 8) for _ in range(200)]
        got = [r for r in pool.map(lambda ab: both_modes("sparse", ab[0], ab[1], fam.is_sparse), cands) if r]
        got.sort(key=lambda r: -r["exact"][2])   # the deepest trees first: they reach the deep stack levels
        have = {mode: sum(1 for r in rows if r["empties"] == e and r[mode]) for mode in ("exact", "wld")}
        need = max(ROWS_MIN, ROWS_MIN + ROWS_MIN - min(have.values()))
        filled[str(e)] = dict(random_exact=have["exact"], random_wld=have["wld"], sparse=min(need, len(got)))
        rows += got[:need]

    # ---- pass chains and early ends, from sparse-ish boards of 6 .. 16 empties
    rs = np.random.RandomState(78)
    cands = [sparse_board(rs, int(rs.randint(6, 17)), 12) for _ in range(3000)]
    names = ("pass2", "rootpass", "passend", "over1")

    def classify(ab):
        r = both_modes("x", ab[0], ab[1], lambda r: r["exact"][2] <= 200000)
        return r and dict(r, family=[name for name in names if fam.CHECKS[name](r)])

    want = dict(pass2=16, rootpass=16, passend=16, over1=16)
    for r in pool.map(classify, cands):
        for name in (r["family"] if r else []):
            if want[name] > 0:
                rows.append(dict(r, family=name))
                want[name] -= 1
                break
    assert not any(want.values()), want

    # ---- games over at the root
    def cols(cs):
        return sum(1 << (8 * r + c) for r in range(8) for c in cs)

    half = 0xFFFFFFFF                                     # rows 0 .. 3
    over = [(cols([0, 1, 2]), cols([5, 6, 7])),            # sealed off: 16 empties, 0
            (cols([0, 1, 2, 3]), cols([6, 7])),            # sealed off: 16 empties, +16
            (cols([6, 7]), cols([0, 1, 2, 3])),            # sealed off: 16 empties, -16
            (cols([0, 1, 2]) | cols([3]) & half, cols([5, 6, 7]) | cols([4]) & ~half & FULL),   # sealed off: 8 empties
            (cols([0, 1, 2, 3, 4, 5]), 0), (0, cols([0, 1, 2, 3, 4, 5])),    # wipe-outs: 16 empties, +48, -48
            (FULL & ~cols([3, 4]) | 1 << 3, 0),                              # wipe-out: 15 empties
            (FULL, 0), (0, FULL), (cols([0, 1, 2, 3]), cols([4, 5, 6, 7])),  # full boards: +64, -64, 0
            (FULL & ~1 & ~(1 << 8), 1 << 8), (1 << 8, FULL & ~1 & ~(1 << 8))]   # the last square: +64, -64 (a pass)
    for a, b in over:
        rows.append(solve_row("over", a, b))
    assert {r["exact"][0] for r in rows if r["family"] == "over"} >= {64, -64, 0}

    # ---- ties at the root and the symmetry bases, from random games
    own, opp = ref.late_positions(1500, 79, 11, 13)
    got = [r for r in pool.map(lambda ab: solve_row("ties", ab[0], ab[1], values=True), list(zip(own, opp)))
           if r and fam.is_tie(r)]
    assert len(got) >= 12, len(got)
    rows += got[:24]
    own, opp = ref.late_positions(200, 80, 12, 16)
    per = {e: 0 for e in range(12, 17)}
    for r in pool.map(lambda ab: solve_row("sym", ab[0], ab[1], values=True), list(zip(own, opp))):
        if r and r["wld"] and per[r["empties"]] < (24 if r["empties"] <= 14 else 12):
            per[r["empties"]] += 1
            rows.append(r)
    assert sum(per.values()) >= 64, per

    # ---- every family has its property, every count its rows
    fam.check_fixture(dict(n_cap=N_CAP, rows_min=ROWS_MIN, filled=filled, rows=rows))
    with open(os.path.join(HERE, "endgame_deep.json"), "w") as f:
        f.write('{"n_cap": %d, "rows_min": %d, "filled": %s, "rows": [\n' % (N_CAP, ROWS_MIN, json.dumps(filled, sort_keys=True)))
        f.write(",\n".join(json.dumps(r, sort_keys=True) for r in rows))
        f.write("\n]}\n")
    print("rows", len(rows), "families", {k: sum(1 for r in rows if r["family"] == k) for k in fam.FAMILIES})
    for e in range(11, 21):
        rr = [r for r in rows if r["empties"] == e]
        print("empties", e, "exact rows", sum(1 for r in rr if r["exact"]), "wld rows", sum(1 for r in rr if r["wld"]),
              "max nodes", max([r["exact"][2] for r in rr if r["exact"]] + [0]),
              max([r["wld"][2] for r in rr if r["wld"]] + [0]),
              "random candidates: %d in %.1f s" % (timing[e][1], timing[e][0]))
    print("filled", filled, "total %.0f s" % (time.time() - t_start))


if __name__ == "__main__":
    main()
