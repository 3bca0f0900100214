"""The fixed-depth alpha-beta opponent (iago_alphabeta_moves, ops.alphabeta_moves) and the opening draw
(iago_random_moves, ops.random_moves) on the device, bit for bit against tests/alphabeta_ref.py: (score, move, done) at
depths 1 to 6, the exact solver where the depth reaches the end of the game, every batch shape around a wave, the node
counts, the refusals and the give-up."""
import numpy as np
import pytest
import torch

from iago_amd import _lib, ops

from . import alphabeta_ref as ab
from . import endgame_ref as er

pytestmark = pytest.mark.gpu

START_OWN, START_OPP = 0x0000000810000000, 0x0000001008000000


def _run(own, opp, depth, **kw):
    r = ops.alphabeta_moves(ops.bits_to_tensor(own), ops.bits_to_tensor(opp), depth, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def _depth_1_tree(own, opp):
    """(legal moves of the side that moves at the root, passes) of a position's depth-1 tree by the reference's rules:
    a pass is a root that must pass, or a leaf whose mover must pass with the game going on.  (0, 0): the game is over."""
    passes = 0
    if not er.bit_legal(own, opp):
        if not er.bit_legal(opp, own):
            return 0, 0
        own, opp, passes = opp, own, 1
    moves = ab.moves_of(own, opp)
    for m in moves:
        a, b = ab.play(own, opp, m)
        passes += bool(not er.bit_legal(a, b) and er.bit_legal(b, a))
    return len(moves), passes


@pytest.fixture(scope="module")
def positions(golden_rules):
    """64 positions: alphabeta_ref.position_set() (random play from 2 to 56 empties, roots that must pass, finished
    games, a full board, one empty) and 16 of the golden trace."""
    own, opp = ab.position_set()
    go, gp = er.golden_positions(golden_rules["trace"], 0, 60)
    pick = np.linspace(0, len(go) - 1, 16).astype(int)
    own += [int(go[i]) for i in pick]
    opp += [int(gp[i]) for i in pick]
    assert len(own) == 64
    return own, opp


@pytest.fixture(scope="module")
def deep(positions):
    """The 16 positions of depths 5 and 6: the midgame boards of the set with at most 24 empties (the Python reference
    takes seconds per board beyond), every second late one and every second hand-made one."""
    own, opp = positions
    mid = [i for i in range(24) if er.empties(own[i], opp[i]) <= 24][:8]
    idx = mid + list(range(24, 40, 2))[:12 - len(mid)] + [40, 42, 44, 47]
    assert len(idx) == 16 and len(set(idx)) == 16 and len(mid) >= 4
    return idx


@pytest.fixture(scope="module")
def reference(positions, deep):
    """depth -> [(score, move)] of the reference, computed once: all 64 at depths 1 to 4, the 16 of `deep` at 5 and 6."""
    own, opp = positions
    want = {d: [ab.alphabeta(a, b, d) for a, b in zip(own, opp)] for d in (1, 2, 3, 4)}
    for d in (5, 6):
        want[d] = [ab.alphabeta(own[i], opp[i], d) for i in deep]
    return want


@pytest.mark.parametrize("depth", [1, 2, 3, 4])
def test_equals_the_reference(positions, reference, depth):
    own, opp = positions
    r = _run(own, opp, depth)
    assert r["done"].all() and not r["ctl"][[0, 2, 3]].any() and r["ctl"][1] >= 64
    got = list(zip(r["score"].tolist(), r["move"].tolist()))
    assert got == reference[depth]
    assert (r["nodes"] >= 1).all()
    if depth == 1:
        seen = 0
        for i, (a, b) in enumerate(zip(own, opp)):
            legal, passes = _depth_1_tree(a, b)
            seen += passes
            # the root, its leaves and the passes of the position's own tree
            assert r["nodes"][i] <= 1 + legal + passes, i
            # The kernel counts nothing for a pass in place, and at depth 1 nothing is cut off: every value is at most
            # 16400 in size, strictly inside the root's window of +-32767.  So the count is exact.
            assert r["nodes"][i] == 1 + legal, i
        assert seen >= 4


@pytest.mark.parametrize("depth", [5, 6])
def test_equals_the_reference_deeper(positions, reference, deep, depth):
    own, opp = positions
    r = _run([own[i] for i in deep], [opp[i] for i in deep], depth)
    assert r["done"].all() and not r["ctl"][[0, 2, 3]].any()
    assert list(zip(r["score"].tolist(), r["move"].tolist())) == reference[depth]


def test_the_start_position_at_depth_10():
    r = _run([START_OWN], [START_OPP], 10)
    assert r["done"][0] == 1 and not r["ctl"][[0, 2, 3]].any()
    assert int(r["move"][0]) in (19, 26, 37, 44) and abs(int(r["score"][0])) < 10000 and r["nodes"][0] > 1000


def test_depth_to_the_end_is_the_exact_solver(positions):
    own, opp = positions
    for depth in (4, 10):
        keep = [i for i in range(64) if er.empties(own[i], opp[i]) <= depth]
        assert len(keep) >= 12
        o, p = ops.bits_to_tensor([own[i] for i in keep]), ops.bits_to_tensor([opp[i] for i in keep])
        got = ops.alphabeta_moves(o, p, depth)
        ex = ops.solve_endgame(o, p, mode="exact", max_empties=depth)
        s = ex["score"].to(torch.int32)
        assert torch.equal(got["score"].to(torch.int32), 10000 * torch.sign(s) + 100 * s)
        assert torch.equal(got["move"], ex["move"]) and bool(got["done"].all()) and bool(ex["solved"].all())
        assert {-1, -2} <= set(got["move"].tolist())


@pytest.fixture(scope="module")
def singles(positions):
    """(score, move, nodes, done) of every position of the set searched alone, depth 3: 64 one-position launches, once."""
    own, opp = positions
    rows = []
    for a, b in zip(own, opp):
        q = _run([a], [b], 3)
        assert not q["ctl"][[0, 2, 3]].any()
        rows.append((int(q["score"][0]), int(q["move"][0]), int(q["nodes"][0]), int(q["done"][0])))
    return rows


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_batch_shapes(positions, reference, singles, n):
    own, opp = positions
    idx = [(7 * i + 3) % 64 for i in range(n)]
    r = _run([own[i] for i in idx], [opp[i] for i in idx], 3)
    assert r["done"].all() and r["ctl"][1] >= n and not r["ctl"][[0, 2, 3]].any()
    assert list(zip(r["score"].tolist(), r["move"].tolist())) == [reference[3][i] for i in idx]
    # every row is the row of its one-position launch, the node count included
    got = list(zip(r["score"].tolist(), r["move"].tolist(), r["nodes"].tolist(), r["done"].tolist()))
    assert got == [singles[i] for i in idx]


def test_lanes_claim_a_second_position(positions, reference):
    """More positions than a launch has lanes, so that lanes finish a search and claim again: the launch has at most
    CUs x (workgroups resident on a CU) workgroups of one wave, and no CU of this family holds more than 40 waves.  The
    64 positions repeated: every repeat equals the first, node counts included, and the first equals the reference."""
    own, opp = positions
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    reps = cus * 40 + 16
    o, p = ops.bits_to_tensor(own).repeat(reps), ops.bits_to_tensor(opp).repeat(reps)
    r = ops.alphabeta_moves(o, p, 2)
    assert bool(r["done"].all()) and r["ctl"].tolist()[1] >= 64 * reps
    assert list(zip(r["score"][:64].tolist(), r["move"][:64].tolist())) == reference[2]
    for k in ("score", "move", "nodes"):
        rows = r[k].reshape(reps, 64)
        assert torch.equal(rows, rows[:1].expand(reps, 64)), k
    alone = _run(own, opp, 2)
    assert np.array_equal(alone["nodes"], r["nodes"][:64].cpu().numpy())


def test_overlapping_boards_are_refused(positions):
    own, opp = positions
    o, p = list(own[:6]), list(opp[:6])
    o[2] |= p[2] & -p[2]          # one stone on both boards
    p[5] |= o[5] & -o[5]
    with pytest.raises(_lib.IagoError, match="refused") as e:
        ops.alphabeta_moves(ops.bits_to_tensor(o), ops.bits_to_tensor(p), 2)
    assert e.value.result["ctl"][2] == 2
    r = _run(o, p, 2, check_result=False)
    assert r["ctl"][2] == 2 and r["ctl"][0] == 0 and r["done"].tolist() == [1, 1, 0, 1, 1, 0]


def test_give_up_on_its_clock():
    own, opp = er.late_positions(256, 61, 30, 44)
    with pytest.raises(_lib.IagoError, match="gave up"):
        ops.alphabeta_moves(ops.bits_to_tensor(own), ops.bits_to_tensor(opp), 10, time_limit_ms=1)
    r = _run(own, opp, 10, time_limit_ms=1, check_result=False)
    assert r["ctl"][0] != 0 and not r["done"].all()
    # what it did finish is what a launch without the limit finds
    fin = np.flatnonzero(r["done"] == 1)
    if len(fin):
        again = _run(own[fin], opp[fin], 10)
        assert np.array_equal(again["score"], r["score"][fin]) and np.array_equal(again["move"], r["move"][fin])
    # the device is fine afterwards
    s = _run(own[:64], opp[:64], 2)
    assert s["done"].all() and s["ctl"][0] == 0


def test_random_moves_equal_the_reference():
    from oracle import oracle as orc
    n, seed, base = 256, 77, 1000
    for id_mod in (n, n // 2):
        own = [START_OWN] * n
        opp = [START_OPP] * n
        for t in range(8):
            got = ops.random_moves(ops.bits_to_tensor(own), ops.bits_to_tensor(opp), seed, base, id_mod, t).cpu().tolist()
            want = [ab.random_move(own[g], opp[g], seed, g, base, id_mod, t) for g in range(n)]
            assert got == want, (id_mod, t)
            nxt = [ab.play(own[g], opp[g], want[g]) if want[g] >= 0 else (opp[g], own[g]) for g in range(n)]
            own, opp = [a for a, _ in nxt], [b for _, b in nxt]
        assert len(set(zip(own, opp))) > n // 4                      # many different openings
        if id_mod == n // 2:
            assert own[:n // 2] == own[n // 2:] and opp[:n // 2] == opp[n // 2:]
    # a mover without a legal move: -1
    got = ops.random_moves(ops.bits_to_tensor([1, START_OWN]), ops.bits_to_tensor([4, START_OPP]), seed, 0, 2, 3)
    assert got.cpu().tolist()[0] == -1 and got.cpu().tolist()[1] in (19, 26, 37, 44)
