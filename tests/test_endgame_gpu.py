"""The exact endgame solver (iago_solve_endgame, ops.solve_endgame, engine.solve_endgame) on the device: exact against
the Python references of tests/endgame_ref.py where they are fast enough, self-consistent (negamax over the children,
WLD = sign of exact, independent of the batch and of the root split) where they are not, and its refusals and give-up.

What is pinned to what: the oracle-rules negamax (endgame_ref.solve_state) holds the bitboard twin (solve_bits) on the
CPU up to 8 empties; the twin holds the kernel here up to 10; the C reference (oracle/endgame_oracle.c, pinned to both
on the CPU) holds it from 11 to 20 empties through tests/golden/endgame_deep.json, rows of at most 2 M reference nodes,
in tests/test_endgame_deep_gpu.py.  The 12 - 16 consistency test below stays a self-check."""
import numpy as np
import pytest
import torch

from iago_amd import _lib, engine, ops

from . import endgame_ref as ref

pytestmark = pytest.mark.gpu

HANDICAPS = [(c // 8, c % 8) for c in engine.HANDICAP_CELLS]


def _late_handicap(n, seed, lo, hi):
    """Positions of seeded random games from the handicap starts (src/train_rl.py:43-46)."""
    from oracle import oracle as orc
    rs = np.random.RandomState(seed)
    own, opp, g = [], [], 0
    while len(own) < n:
        hc = HANDICAPS[g % 4]
        _, _, tr = orc.random_playout(orc.initial_state(hc), 1, seed=seed, game_id=g)
        g += 1
        s, color, cands = orc.initial_state(hc), 1, []
        for a in tr + [None]:
            p1, p2 = orc.state_to_bits(s)
            if lo <= ref.empties(p1, p2) <= hi:
                cands.append((p1, p2) if color == 1 else (p2, p1))
            if a is None:
                break
            if a != -1:
                orc.place_stone(s, a, color)
            color = 3 - color
        if cands:
            o, p = cands[rs.randint(len(cands))]
            own.append(o)
            opp.append(p)
    return np.array(own, np.uint64), np.array(opp, np.uint64)


def _passers(n, seed):
    """Positions whose side to move must pass (and finished games): swapped sides of positions where the opponent
    has no move."""
    own, opp = [], []
    o, p = ref.late_positions(4 * n, seed, 1, 8)
    for a, b in zip(o, p):
        if ref.bit_legal(int(b), int(a)) == 0:
            own.append(b)
            opp.append(a)
        if len(own) == n:
            break
    return np.array(own, np.uint64), np.array(opp, np.uint64)


def _solve(own, opp, mode="exact", **kw):
    r = ops.solve_endgame(ops.bits_to_tensor(own), ops.bits_to_tensor(opp), mode=mode, **kw)
    return {k: v.cpu().numpy() for k, v in r.items()}


@pytest.fixture(scope="module")
def small(golden_rules):
    parts = [ref.golden_positions(golden_rules["trace"], 0, 8), ref.late_positions(760, 11, 0, 8),
             _late_handicap(300, 12, 0, 8), _passers(60, 13)]
    own = np.concatenate([p[0] for p in parts])
    opp = np.concatenate([p[1] for p in parts])
    return own, opp


def test_exact_matches_reference_up_to_8_empties(small):
    own, opp = small
    assert len(own) >= 1900
    r = _solve(own, opp)
    assert r["solved"].all() and r["ctl"][0] == 0 and r["ctl"][2] == 0
    seen = set()
    for i, (a, b) in enumerate(zip(own, opp)):
        want = ref.solve_bits(a, b)
        assert (int(r["score"][i]), int(r["move"][i])) == want, (i, hex(int(a)), hex(int(b)))
        seen.add(want[1] if want[1] < 0 else 0)
    assert seen == {0, -1, -2}   # moves, passes and finished games all covered


def test_wld_matches_reference_up_to_8_empties(small):
    own, opp = small
    r = _solve(own, opp, mode="wld")
    assert r["solved"].all() and r["ctl"][0] == 0
    for i, (a, b) in enumerate(zip(own, opp)):
        assert (int(r["score"][i]), int(r["move"][i])) == ref.solve_bits(a, b, wld=True), i


def test_exact_matches_reference_at_10_empties(golden_rules):
    go, gp = ref.golden_positions(golden_rules["trace"], 10, 10)
    so, sp = ref.late_positions(25, 21, 10, 10)
    own, opp = np.concatenate([go[:25], so]), np.concatenate([gp[:25], sp])
    r = _solve(own, opp, max_empties=10)
    assert r["solved"].all() and r["ctl"][0] == 0
    for i, (a, b) in enumerate(zip(own, opp)):
        assert (int(r["score"][i]), int(r["move"][i])) == ref.solve_bits(a, b), i


@pytest.fixture(scope="module")
def deep():
    return ref.late_positions(500, 31, 12, 16)


def test_negamax_consistency_12_to_16_empties(deep):
    own, opp = deep
    r = _solve(own, opp)
    w = _solve(own, opp, mode="wld")
    assert r["solved"].all() and r["ctl"][0] == 0 and w["solved"].all()
    assert (w["score"] == np.sign(r["score"])).all()
    # every child of every position, in one launch
    kids, owner = [], []
    for i, (a, b) in enumerate(zip(own, opp)):
        a, b = int(a), int(b)
        ms = ref.BitRules.moves((a, b))
        for m in ms:
            kids.append((m,) + ref.BitRules.play((a, b), m))
            owner.append(i)
        if not ms:
            kids.append((-1, b, a))
            owner.append(i)
    c = _solve(np.array([k[1] for k in kids], np.uint64), np.array([k[2] for k in kids], np.uint64))
    assert c["solved"].all()
    best = {}
    for j, (m, _, _) in enumerate(kids):
        i, v = owner[j], -int(c["score"][j])
        if i not in best or v > best[i][0]:
            best[i] = (v, m)
    for i in range(len(own)):
        assert (int(r["score"][i]), int(r["move"][i])) == best[i], i
    # WLD: the lowest index of the best outcome
    for i in range(len(own)):
        sgn = [(-np.sign(int(c["score"][j])), kids[j][0]) for j in range(len(kids)) if owner[j] == i]
        top = max(s for s, _ in sgn)
        assert int(w["move"][i]) == min(m for s, m in sgn if s == top), i


def test_batch_independence(deep):
    own, opp = deep
    base = _solve(own, opp)
    perm = np.random.RandomState(5).permutation(len(own))
    sh = _solve(own[perm], opp[perm])
    for k in ("score", "move", "nodes"):
        assert (sh[k] == base[k][perm]).all(), k
    reps = np.arange(4096) % len(own)
    big = _solve(own[reps], opp[reps])
    for k in ("score", "move", "nodes"):
        assert (big[k] == base[k][reps]).all(), k
    for i in range(0, len(own), 100):
        one = _solve(own[i:i + 1], opp[i:i + 1])
        for k in ("score", "move", "nodes"):
            assert one[k][0] == base[k][i], (k, i)


@pytest.mark.parametrize("split", [1, 2, 3])
@pytest.mark.parametrize("mode", ["exact", "wld"])
def test_root_split_equals_plain(split, mode):
    own, opp = ref.late_positions(6, 33 + split, 12, 13)
    base = _solve(own, opp, mode=mode)
    for j, i in enumerate(range(len(own))):
        o, p = ops.bits_to_tensor(own[i:i + 1]), ops.bits_to_tensor(opp[i:i + 1])
        r = engine.solve_endgame(o, p, mode=mode, split_depth=split)
        assert int(r["score"][0].item()) == base["score"][j] and int(r["move"][0].item()) == base["move"][j], (i, split)
        assert int(r["solved"][0].item()) == 1


def test_root_split_of_a_batch_with_passes_and_ends():
    own, opp = _passers(12, 41)
    o2, p2 = ref.late_positions(12, 42, 9, 12)
    own, opp = np.concatenate([own, o2]), np.concatenate([opp, p2])
    base = _solve(own, opp)
    for split in (1, 3):
        r = engine.solve_endgame(ops.bits_to_tensor(own), ops.bits_to_tensor(opp), split_depth=split)
        assert (r["score"].cpu().numpy() == base["score"]).all() and (r["move"].cpu().numpy() == base["move"]).all()


def test_refusals():
    full = 0xFFFFFFFF00000000
    o, p = ref.late_positions(4, 51, 6, 6)
    own = np.array([o[0], o[1], full, o[2], o[3]], np.uint64)
    opp = np.array([p[0], p[1], full | 1, 0, p[3]], np.uint64)   # row 2 overlaps, row 3 has 63 empties
    with pytest.raises(_lib.IagoError) as e:
        ops.solve_endgame(ops.bits_to_tensor(own), ops.bits_to_tensor(opp))
    r = {k: v.cpu().numpy() for k, v in e.value.result.items()}
    assert r["ctl"][2] == 2 and r["ctl"][0] == 0
    assert list(r["solved"]) == [1, 1, 0, 0, 1]
    # more empties than max_empties: refused by the launch, the others solved
    with pytest.raises(_lib.IagoError):
        ops.solve_endgame(ops.bits_to_tensor(o), ops.bits_to_tensor(p), max_empties=5)
    r = _solve(o, p, max_empties=5, check_result=False)
    assert r["ctl"][2] == 4 and not r["solved"].any()
    for bad in (dict(max_empties=21), dict(max_empties=-1), dict(time_limit_ms=0), dict(mode="best")):
        with pytest.raises((_lib.IagoError, ValueError)):
            _solve(o, p, **bad)


def test_give_up_on_its_clock():
    own, opp = ref.late_positions(256, 61, 20, 20)
    with pytest.raises(_lib.IagoError, match="gave up"):
        ops.solve_endgame(ops.bits_to_tensor(own), ops.bits_to_tensor(opp), time_limit_ms=1)
    r = _solve(own, opp, time_limit_ms=1, check_result=False)
    assert r["ctl"][0] != 0
    assert not r["solved"].all()
    # the device is fine afterwards
    small_o, small_p = ref.late_positions(64, 62, 4, 6)
    s = _solve(small_o, small_p)
    assert s["solved"].all() and s["ctl"][0] == 0
