"""The root split of the exact solver on the device (iago_solve_endgame_split, ops.solve_endgame(split=),
ops.solve_endgame_moves(split=)), bit for bit: score, move and solved against the unsplit launch, the best set and the
per-move row against ops.solve_endgame_moves(moves="all"), the job arrays and the node counts against the restatement
(tests/endgame_split_ref.py), deep rows against the independent C reference's fixture, batch shapes around a wave and
past one round of the scan, the count-only form, the capacity and its overflow, the refusals, the give-up, the default,
and the two callers that pass the split through.  Every launch runs under an explicit time_limit_ms and asserts that it
neither gave up (ctl[0]) nor ran out of stack (ctl[3])."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from iago_amd import _lib, engine, ops

from . import endgame_ref as er
from . import endgame_split_ref as sr
from .conftest import load_json

pytestmark = pytest.mark.gpu

MODES = ("exact", "wld")
SPLITS = (1, 2)
CASES = [(m, s) for m in MODES for s in SPLITS]
LIMIT_MS = 20000            # positions of at most 10 empties: milliseconds of device time
LANE_NODES_PER_S = 0.4e6    # tests/test_endgame_deep_gpu.py's clock rule
NO_MOVE = _lib.ENDGAME_NO_MOVE
PASS_FAMILIES = ("pass2", "rootpass", "passend", "over", "over1")
JOB_ARRAYS = (("job_own", torch.int64, 1), ("job_opp", torch.int64, 1), ("job_root", torch.int32, 1),
              ("job_path", torch.int8, 4), ("job_score", torch.int8, 1), ("job_move", torch.int8, 1),
              ("job_nodes", torch.int64, 1), ("job_done", torch.uint8, 1))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _np(r):
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}


def _u(x):
    return int(x) & 0xFFFFFFFFFFFFFFFF


def _ok(r, n=None):
    """What every launch asserts: no give-up, no stack overflow; and (n given) everything solved, nothing refused."""
    assert r["ctl"][0] == 0, "gave up"
    assert r["ctl"][3] == 0, "out of stack"
    if n is not None:
        assert r["ctl"][2] == 0 and len(r["solved"]) == n and r["solved"].all()
    return r


def _split(own, opp, mode, split, moves="all", limit_ms=LIMIT_MS, **kw):
    return _np(ops.solve_endgame_moves(ops.bits_to_tensor(own), ops.bits_to_tensor(opp), mode=mode, moves=moves,
                                       split=split, time_limit_ms=limit_ms, **kw))


def _plain(own, opp, mode, limit_ms=LIMIT_MS, **kw):
    return _np(ops.solve_endgame(ops.bits_to_tensor(own), ops.bits_to_tensor(opp), mode=mode, time_limit_ms=limit_ms,
                                 **kw))


@pytest.fixture(scope="module")
def fx():
    return load_json("endgame_deep.json")


@pytest.fixture(scope="module")
def positions(fx):
    """48 late positions of 0 - 9 empties, the hand-made roots, the root whose child must pass, and the fixture's
    pass / early-end rows of at most 10 empties."""
    own, opp = sr.position_set(48, 9)
    rows = [r for r in fx["rows"] if r["family"] in PASS_FAMILIES and r["empties"] <= 10]
    assert {r["family"] for r in rows} == set(PASS_FAMILIES)
    own, opp = own + [r["own"] for r in rows], opp + [r["opp"] for r in rows]
    assert set().union(*[sr.kinds_of(a, b) for a, b in zip(own[:54], opp[:54])]) == sr.KINDS
    assert max(er.empties(a, b) for a, b in zip(own, opp)) == 10 and len(own) % 64 != 0
    return own, opp


@pytest.fixture(scope="module")
def want(positions):
    """(mode, split) -> the restatement's answer per root, computed once."""
    own, opp = positions
    return {(m, s): [sr.split_solve(a, b, s, m == "wld") for a, b in zip(own, opp)] for m, s in CASES}


@pytest.fixture(scope="module")
def runs(positions):
    """(mode, split) -> the split launch of the positions with every output (exact capacity from a count-only launch)."""
    own, opp = positions
    return {(m, s): _ok(_split(own, opp, m, s, max_empties=10), len(own)) for m, s in CASES}


@pytest.fixture(scope="module")
def unsplit(positions):
    own, opp = positions
    return {m: _ok(_np(ops.solve_endgame_moves(ops.bits_to_tensor(own), ops.bits_to_tensor(opp), mode=m, moves="all",
                                               max_empties=10, time_limit_ms=LIMIT_MS)), len(own)) for m in MODES}


# ---------------------------------------------------------------- equal to the unsplit search
@pytest.mark.parametrize("mode,split", CASES)
def test_results_equal_the_unsplit_search(positions, runs, unsplit, mode, split):
    own, opp = positions
    r, u = runs[(mode, split)], unsplit[mode]
    plain = _ok(_plain(own, opp, mode, max_empties=10), len(own))
    assert len(r["ctl"]) == 8 and not r["ctl"][[2, 6, 7]].any()
    for k in ("score", "move", "solved"):
        assert np.array_equal(r[k], plain[k]) and r[k].dtype == plain[k].dtype, k
    for k in ("score", "move", "best", "move_score"):
        assert np.array_equal(r[k], u[k]) and r[k].dtype == u[k].dtype, k
    assert {-1, -2} <= set(r["move"].tolist())
    assert r["jobs"] == r["job_capacity"] == int(r["job_count"].sum()) == r["ctl"][4] and r["ctl"][5] == 0
    assert r["ctl"][1] >= r["jobs"]            # every job was claimed
    # the two other forms of the call: no optional output, the set alone
    a = _ok(_np(ops.solve_endgame(ops.bits_to_tensor(own), ops.bits_to_tensor(opp), mode=mode, max_empties=10,
                                  time_limit_ms=LIMIT_MS, split=split)), len(own))
    b = _ok(_split(own, opp, mode, split, moves="best", max_empties=10), len(own))
    assert "best" not in a and "move_score" not in a and "move_score" not in b
    for k in ("score", "move", "nodes", "job_score", "job_nodes"):
        assert np.array_equal(a[k], r[k]) and np.array_equal(b[k], r[k]), k
    assert np.array_equal(b["best"], r["best"])


@pytest.mark.parametrize("mode,split", CASES)
def test_the_jobs_and_the_nodes_are_the_restatements(runs, want, mode, split):
    r, w = runs[(mode, split)], want[(mode, split)]
    counts = [len(x["jobs"]) for x in w]
    assert r["job_count"].tolist() == counts
    assert r["job_first"].tolist() == (np.cumsum(counts) - counts).tolist()
    flat = [(i,) + j + v for i, x in enumerate(w) for j, v in zip(x["jobs"], x["job_values"])]
    assert len(flat) == r["jobs"]
    got = [(int(r["job_root"][j]), _u(r["job_own"][j]), _u(r["job_opp"][j])) + tuple(int(x) for x in r["job_path"][j, :3])
           + (int(r["job_score"][j]), int(r["job_move"][j]), int(r["job_nodes"][j])) for j in range(r["jobs"])]
    assert got == flat
    assert not r["job_path"][:, 3].any() and r["job_done"].all()
    assert r["nodes"].tolist() == [x["nodes"] for x in w]
    assert r["score"].tolist() == [x["score"] for x in w] and r["move"].tolist() == [x["move"] for x in w]
    assert [_u(b) for b in r["best"]] == [x["best"] for x in w]
    assert r["move_score"].tolist() == [x["row"] for x in w]


# ---------------------------------------------------------------- against the independent C reference
def _deep_limit_ms(fx):
    return int(4 * 1000 * fx["n_cap"] / LANE_NODES_PER_S)


def _fixture_rows(fx):
    """The rows tests/test_endgame_deep_gpu.py::test_split_against_the_fixture selects."""
    both = [r for r in fx["rows"] if r["exact"] and r["wld"]]
    rows = []
    for e in range(12, 17):
        rows += sorted((r for r in both if r["family"] in ("random", "sym") and r["empties"] == e),
                       key=lambda r: r["exact"][3])[:3]
    assert len(rows) == 15
    for f in PASS_FAMILIES:
        rows += [r for r in both if r["family"] == f][:6]
    return rows


@pytest.mark.parametrize("mode,split", CASES)
def test_against_the_fixture(fx, mode, split):
    rows = _fixture_rows(fx)
    assert len(rows) == 45 and {r["family"] for r in rows} >= set(PASS_FAMILIES)
    own, opp = [r["own"] for r in rows], [r["opp"] for r in rows]
    r = _ok(_split(own, opp, mode, split, moves="best", limit_ms=_deep_limit_ms(fx), max_empties=16), len(rows))
    for i, row in enumerate(rows):
        assert (int(r["score"][i]), int(r["move"][i])) == tuple(row[mode][:2]), (i, row["family"], row["empties"])


@pytest.mark.parametrize("mode,split", CASES)
def test_move_values_against_the_fixture(fx, mode, split):
    """Every move's value on the ties and sym rows: the fixture's, which owe nothing to any solver's move order."""
    rows = [r for r in fx["rows"] if r["family"] in ("ties", "sym") and r["empties"] <= 13 and r[mode]]
    assert len(rows) >= 60 and {r["family"] for r in rows} == {"ties", "sym"}
    own, opp = [r["own"] for r in rows], [r["opp"] for r in rows]
    r = _ok(_split(own, opp, mode, split, limit_ms=_deep_limit_ms(fx), max_empties=13), len(rows))
    for i, row in enumerate(rows):
        vals = {int(m): (v if mode == "exact" else (v > 0) - (v < 0)) for m, v in row["values"].items()}
        assert r["move_score"][i].tolist() == [vals.get(a, NO_MOVE) for a in range(64)], i
        top = max(vals.values())
        assert int(r["score"][i]) == top == row[mode][0]
        assert _u(r["best"][i]) == sum(1 << m for m, v in vals.items() if v == top)
        assert int(r["move"][i]) == min(m for m, v in vals.items() if v == top) == row[mode][1]


# ---------------------------------------------------------------- shapes
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 130])
def test_batch_shapes(positions, runs, n):
    own, opp = positions
    whole = runs[("exact", 2)]
    idx = [(7 * i + 3) % len(own) for i in range(n)]
    r = _ok(_split([own[i] for i in idx], [opp[i] for i in idx], "exact", 2, max_empties=10), n)
    for k in ("score", "move", "nodes", "best", "move_score", "job_count"):
        assert np.array_equal(r[k], whole[k][idx]), k
    assert r["jobs"] == whole["job_count"][idx].sum() and r["move_score"].shape == (n, 64)


def test_a_root_alone_and_inside_a_batch(positions, runs):
    own, opp = positions
    for mode, split in CASES:
        whole = runs[(mode, split)]
        for i in (5, 50, 53, len(own) - 1):     # a late one, a hand-made one, the child that must pass, a fixture row
            r = _ok(_split(own[i:i + 1], opp[i:i + 1], mode, split, max_empties=10), 1)
            for k in ("score", "move", "nodes", "best", "move_score", "job_count"):
                assert np.array_equal(r[k], whole[k][i:i + 1]), (k, i)
            j0, c = int(whole["job_first"][i]), int(whole["job_count"][i])
            for k in ("job_own", "job_opp", "job_path", "job_score", "job_move", "job_nodes"):
                assert np.array_equal(r[k], whole[k][j0:j0 + c]), (k, i)


def test_more_roots_than_one_round_of_the_scan():
    """1030 roots of 0 - 4 empties: the scan's second round (roots 1024 ..) carries the first round's total."""
    o, p = er.late_positions(103, 83, 0, 4)
    own, opp = np.tile(o, 10), np.tile(p, 10)
    counts = [len(sr.jobs_of(a, b, 2)) for a, b in zip(o, p)] * 10
    r = _ok(_split(own, opp, "exact", 2, max_empties=4), 1030)
    u = _ok(_np(ops.solve_endgame_moves(ops.bits_to_tensor(own), ops.bits_to_tensor(opp), moves="all", max_empties=4,
                                        time_limit_ms=LIMIT_MS)), 1030)
    assert r["job_count"].tolist() == counts and sum(counts[:1024]) > 0
    assert r["job_first"].tolist() == (np.cumsum(counts) - counts).tolist()
    assert r["jobs"] == sum(counts) and r["job_root"].tolist() == [i for i, c in enumerate(counts) for _ in range(c)]
    for k in ("score", "move", "best", "move_score"):
        assert np.array_equal(r[k], u[k]), k
    assert np.array_equal(r["nodes"][:103], r["nodes"][927:])


# ---------------------------------------------------------------- capacity
def _raw(own, opp, split, capacity, max_empties=10, guard=0, count_only=False, fill=0x5A):
    """The C call with the test's own arrays: every array holds its rows + guard rows filled with `fill` (no job arrays
    at all with count_only).  Returns the return code and the arrays as numpy."""
    n = len(own)
    dev = "cuda"
    t = dict(own=ops.bits_to_tensor(own), opp=ops.bits_to_tensor(opp),
             score=torch.full((n + guard,), fill, dtype=torch.int8, device=dev),
             move=torch.full((n + guard,), fill, dtype=torch.int8, device=dev),
             nodes=torch.full((n + guard,), fill, dtype=torch.int64, device=dev),
             solved=torch.full((n + guard,), fill, dtype=torch.uint8, device=dev),
             best=torch.full((n + guard,), fill, dtype=torch.int64, device=dev),
             move_score=torch.full(((n + guard) * 64,), fill, dtype=torch.int8, device=dev),
             job_count=torch.full((n + guard,), fill, dtype=torch.int32, device=dev),
             job_first=torch.full((n + guard,), fill, dtype=torch.int64, device=dev),
             ctl=torch.full((8 + guard,), fill, dtype=torch.int32, device=dev))
    a = _lib.EndgameSplitArgs()
    a.n, a.mode, a.split, a.max_empties, a.time_limit_ms, a.job_capacity = n, 0, split, max_empties, LIMIT_MS, capacity
    if not count_only:
        for k, dt, cols in JOB_ARRAYS:
            t[k] = torch.full(((capacity + guard) * cols,), fill, dtype=dt, device=dev)
    for k, v in t.items():
        if not (count_only and k in ("score", "move", "nodes", "solved", "best", "move_score")):
            setattr(a, k, v.data_ptr())
    rc = _lib.lib().iago_solve_endgame_split(C.byref(a), None)
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in t.items()}


def test_count_only(positions, want):
    own, opp = positions
    n = len(own)
    for split in SPLITS:
        rc, t = _raw(own, opp, split, 0, guard=4, count_only=True)
        assert rc == 0
        counts = [len(x["jobs"]) for x in want[("exact", split)]]
        assert t["job_count"][:n].tolist() == counts
        assert t["job_first"][:n].tolist() == (np.cumsum(counts) - counts).tolist()
        assert t["ctl"][:8].tolist() == [0, 0, 0, 0, sum(counts), 0, 0, 0]
        # nothing else was launched or written
        for k in ("score", "move", "nodes", "solved", "best", "move_score"):
            assert (t[k] == 0x5A).all(), k
        for k in ("job_count", "job_first", "ctl"):
            assert (t[k][-4:] == 0x5A).all(), k


def test_an_exact_capacity_and_one_short(positions, runs):
    own, opp = positions
    n = len(own)
    whole = runs[("exact", 2)]
    need = whole["jobs"]
    r = _ok(_split(own, opp, "exact", 2, max_empties=10, job_capacity=need), n)
    assert r["ctl"][6] == 0 and r["jobs"] == need
    for k in ("score", "move", "nodes", "best", "move_score", "job_own", "job_opp", "job_path", "job_score", "job_nodes"):
        assert np.array_equal(r[k], whole[k]), k
    guard = 64
    rc, t = _raw(own, opp, 2, need, guard=guard)
    assert rc == 0 and t["ctl"][0] == t["ctl"][3] == 0 and t["ctl"][6] == 0 and t["solved"][:n].all()
    assert np.array_equal(t["score"][:n], whole["score"]) and np.array_equal(t["move"][:n], whole["move"])
    assert np.array_equal(t["best"][:n], whole["best"])
    assert np.array_equal(t["move_score"][:n * 64].reshape(n, 64), whole["move_score"])
    for k, _, cols in JOB_ARRAYS:
        assert (t[k][need * cols:] == 0x5A).all(), k
    for k in ("score", "move", "nodes", "solved", "best", "job_count", "job_first", "ctl"):
        assert (t[k][-guard:] == 0x5A).all(), k
    assert (t["move_score"][n * 64:] == 0x5A).all()
    # one job short: nothing is searched
    with pytest.raises(_lib.IagoError, match="job_capacity") as e:
        ops.solve_endgame(ops.bits_to_tensor(own), ops.bits_to_tensor(opp), max_empties=10, time_limit_ms=LIMIT_MS,
                          split=2, job_capacity=need - 1)
    assert e.value.jobs_needed == need and str(need) in str(e.value)
    r = _split(own, opp, "exact", 2, max_empties=10, job_capacity=need - 1, check_result=False)
    assert r["ctl"][0] == r["ctl"][3] == 0
    assert r["ctl"][6] != 0 and r["ctl"][4] == need and r["ctl"][5] == 0 and not r["solved"].any()
    assert r["ctl"][1] == 0                                   # nothing was claimed: nothing was searched
    rc, t = _raw(own, opp, 2, need - 1, guard=guard)
    assert rc == 0 and t["ctl"][6] != 0 and t["ctl"][4] == need and t["ctl"][0] == t["ctl"][3] == 0
    assert not t["solved"][:n].any() and t["job_count"][:n].tolist() == whole["job_count"].tolist()
    for k, _, cols in JOB_ARRAYS:
        assert (t[k][(need - 1) * cols:] == 0x5A).all(), k
    for k in ("score", "move", "nodes", "solved", "best", "job_count", "job_first", "ctl"):
        assert (t[k][-guard:] == 0x5A).all(), k


# ---------------------------------------------------------------- refusals
def test_refused_roots_in_the_middle_of_a_wave(positions, runs):
    own, opp = positions
    o, p = list(own[:40]), list(opp[:40])
    o[17] |= p[17] & -p[17]                       # one stone on both boards
    xo, xp = er.late_positions(1, 511, 10, 10)    # max_empties + 1 empties
    o[29], p[29] = int(xo[0]), int(xp[0])
    assert er.empties(o[29], p[29]) == 10
    with pytest.raises(_lib.IagoError, match="refused") as e:
        ops.solve_endgame_moves(ops.bits_to_tensor(o), ops.bits_to_tensor(p), moves="all", max_empties=9, split=2,
                                time_limit_ms=LIMIT_MS)
    assert e.value.result["ctl"][2] == 2
    r = _ok(_split(o, p, "exact", 2, max_empties=9, check_result=False))
    assert r["ctl"][2] == 2 and r["ctl"][6] == 0
    assert r["solved"].tolist() == [0 if i in (17, 29) else 1 for i in range(40)]
    assert r["job_count"][[17, 29]].tolist() == [0, 0] and r["best"][[17, 29]].tolist() == [0, 0]
    assert (r["move_score"][[17, 29]] == NO_MOVE).all()
    keep = [i for i in range(40) if i not in (17, 29)]
    for k in ("score", "move", "nodes", "best", "move_score", "job_count"):
        assert np.array_equal(r[k][keep], runs[("exact", 2)][k][keep]), k


# ---------------------------------------------------------------- the clock
def test_give_up_on_its_clock(fx):
    deep = [r for r in fx["rows"] if r["empties"] >= 18 and r["wld"]][:6]
    light = [r for r in fx["rows"] if r["family"] == "over" and r["wld"]][:4]    # finished games: solved at once
    rows = light + deep
    assert len(deep) == 6 and len(light) == 4
    own, opp = [r["own"] for r in rows], [r["opp"] for r in rows]
    with pytest.raises(_lib.IagoError, match="gave up"):
        ops.solve_endgame(ops.bits_to_tensor(own), ops.bits_to_tensor(opp), mode="wld", time_limit_ms=1, split=2)
    r = _split(own, opp, "wld", 2, limit_ms=1, check_result=False)
    assert r["ctl"][0] != 0 and r["ctl"][3] == 0 and r["ctl"][6] == 0 and not r["solved"].all()
    for i, row in enumerate(rows):
        if r["solved"][i]:
            assert (int(r["score"][i]), int(r["move"][i])) == tuple(row["wld"][:2]), i
    # a root is solved only with all of its jobs
    first, count = r["job_first"], r["job_count"]
    for i in range(len(rows)):
        assert r["solved"][i] == r["job_done"][first[i]:first[i] + count[i]].all(), i
    # the device is fine afterwards
    s = _ok(_split(own[:4], opp[:4], "wld", 2), 4)
    assert [(int(a), int(b)) for a, b in zip(s["score"], s["move"])] == [tuple(row["wld"][:2]) for row in light]


# ---------------------------------------------------------------- the default, and the callers
def test_split_0_is_the_call_without_the_argument(positions):
    own, opp = positions
    o, p = ops.bits_to_tensor(own), ops.bits_to_tensor(opp)
    a = _ok(_np(ops.solve_endgame(o, p, max_empties=10, time_limit_ms=LIMIT_MS)), len(own))
    b = _ok(_np(ops.solve_endgame(o, p, max_empties=10, time_limit_ms=LIMIT_MS, split=0, job_capacity=None)), len(own))
    assert sorted(a) == sorted(b) == ["ctl", "move", "nodes", "score", "solved"] and len(a["ctl"]) == 4
    c = _ok(_np(ops.solve_endgame_moves(o, p, moves="all", max_empties=10, time_limit_ms=LIMIT_MS)), len(own))
    d = _ok(_np(ops.solve_endgame_moves(o, p, moves="all", max_empties=10, time_limit_ms=LIMIT_MS, split=0)), len(own))
    assert sorted(c) == sorted(d) == ["best", "ctl", "move", "move_score", "nodes", "score", "solved"]
    for x, y in ((a, b), (c, d)):
        for k in x:
            assert np.array_equal(x[k], y[k]) and x[k].dtype == y[k].dtype, k


def test_endgame_errors_passes_the_split_through():
    o, p = er.late_positions(64, 91, 1, 8)
    own, opp, move = [], [], []
    for a, b in zip(o, p):                        # every position with up to four of its moves, or its pass
        legal = sr.moves_of(int(a), int(b)) or [-1]
        for k in range(4):
            own.append(int(a))
            opp.append(int(b))
            move.append(legal[(3 * k) % len(legal)])
    assert len(own) == 256
    t = (ops.bits_to_tensor(own), ops.bits_to_tensor(opp), torch.tensor(move, dtype=torch.int64, device="cuda"))
    a = engine.endgame_errors(*t, max_empties=8, time_limit_ms=LIMIT_MS)
    b = engine.endgame_errors(*t, max_empties=8, time_limit_ms=LIMIT_MS, split=2)
    assert a["rows"] == b["rows"] > 200 and sorted(a) == sorted(b)
    for k, v in a.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(v, b[k]), k
        else:
            assert v == b[k], k


def test_value_labels_pass_the_split_through():
    from iago_amd import network, value_self_play
    policy = network.SLPolicy().load_npz(os.path.join(GOLDEN, "sl_model.npz")).cuda().eval()
    stop = torch.from_numpy(np.random.RandomState(4).randint(54, 64, 64))
    a = value_self_play.generate(policy, policy, 64, stop_num=stop, seed=11, exact_empties=8)
    b = value_self_play.generate(policy, policy, 64, stop_num=stop, seed=11, exact_empties=8, exact_split=1)
    assert int(a["exact"].sum().item()) > 10 and sorted(a) == sorted(b)
    for k in ("z_exact", "exact", "own", "opp", "z"):
        assert torch.equal(a[k], b[k]), k
