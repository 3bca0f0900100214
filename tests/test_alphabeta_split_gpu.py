"""The root split of the alpha-beta opponent on the device (iago_alphabeta_moves_split, ops.alphabeta_moves(split=)),
bit for bit: (score, move, done) against the unsplit launch and the Python reference, the job arrays against the
restatement (tests/alphabeta_split_ref.py), the node counts against unsplit launches of the jobs, batch shapes around a
wave, the count-only form, the capacity and its overflow, the give-up, the refusal, and matches against
AlphaBeta(depth, split) record for record."""
import ctypes as C

import numpy as np
import pytest
import torch

from iago_amd import _lib, ops

from . import alphabeta_ref as ab
from . import alphabeta_split_ref as sr
from . import endgame_ref as er
from .test_match_alphabeta_gpu import B, BASE, KEYS, N_SIMS, N_THR, OPENING, SEED, nets  # noqa: F401  (that match)

pytestmark = pytest.mark.gpu

CASES = [(2, 1), (3, 1), (3, 2), (4, 1), (4, 2)]
DEEP_CASES = [(5, 1), (6, 2)]
JOB_ARRAYS = (("job_own", torch.int64, 1), ("job_opp", torch.int64, 1), ("job_root", torch.int32, 1),
              ("job_path", torch.int8, 4), ("job_score", torch.int16, 1), ("job_move", torch.int8, 1),
              ("job_nodes", torch.int64, 1), ("job_done", torch.uint8, 1))


def _np(r):
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}


def _run(own, opp, depth, **kw):
    return _np(ops.alphabeta_moves(ops.bits_to_tensor(own), ops.bits_to_tensor(opp), depth, **kw))


def _u(x):
    return int(np.uint64(x))


@pytest.fixture(scope="module")
def positions():
    own, opp = sr.position_set()
    assert len(own) == 49
    return own, opp


@pytest.fixture(scope="module")
def deep(positions):
    """16 of the positions for the deeper cases: the midgame boards of at most 24 empties, late ones, hand-made ones and
    the one whose child must pass."""
    own, opp = positions
    mid = [i for i in range(24) if er.empties(own[i], opp[i]) <= 24][:8]
    idx = mid + list(range(24, 40, 2))[:11 - len(mid)] + [40, 42, 44, 47, 48]
    assert len(idx) == 16 and len(set(idx)) == 16
    return idx


@pytest.fixture(scope="module")
def unsplit(positions):
    """depth -> the unsplit launch of the 49 positions, computed once."""
    own, opp = positions
    return {d: _run(own, opp, d) for d in (2, 3, 4)}


@pytest.fixture(scope="module")
def split_runs(positions):
    """(depth, split) -> the split launch of the 49 positions (exact capacity from a count-only launch), computed once."""
    own, opp = positions
    return {c: _run(own, opp, c[0], split=c[1]) for c in CASES}


@pytest.fixture(scope="module")
def reference(positions):
    own, opp = positions
    return {d: [ab.alphabeta(a, b, d) for a, b in zip(own, opp)] for d in (2, 3, 4)}


@pytest.fixture(scope="module")
def ref_jobs(positions):
    """(depth, split) -> the restatement's jobs per root."""
    own, opp = positions
    return {c: [sr.jobs_of(a, b, c[0], c[1]) for a, b in zip(own, opp)] for c in CASES}


@pytest.mark.parametrize("depth,split", CASES)
def test_results_equal_the_unsplit_search(split_runs, unsplit, reference, depth, split):
    r, u = split_runs[(depth, split)], unsplit[depth]
    assert u["done"].all() and not u["ctl"][[0, 2, 3]].any()
    assert not r["ctl"][[0, 2, 3, 6, 7]].any() and len(r["ctl"]) == 8
    for k in ("score", "move", "done"):
        assert np.array_equal(r[k], u[k]), k
        assert r[k].dtype == u[k].dtype
    assert list(zip(r["score"].tolist(), r["move"].tolist())) == reference[depth]
    assert {-1, -2} <= set(r["move"].tolist())
    assert r["jobs"] == r["job_capacity"] == int(r["job_count"].sum()) == r["ctl"][4] and r["ctl"][5] == 0
    assert r["ctl"][1] >= r["jobs"]            # every job was claimed


@pytest.mark.parametrize("depth,split", DEEP_CASES)
def test_results_equal_the_unsplit_search_deeper(positions, deep, depth, split):
    own, opp = positions
    o, p = [own[i] for i in deep], [opp[i] for i in deep]
    r, u = _run(o, p, depth, split=split), _run(o, p, depth)
    assert u["done"].all() and not r["ctl"][[0, 2, 3, 6]].any()
    for k in ("score", "move", "done"):
        assert np.array_equal(r[k], u[k]), k


@pytest.mark.parametrize("depth,split", CASES)
def test_the_jobs_are_the_restatements(split_runs, ref_jobs, depth, split):
    r, want = split_runs[(depth, split)], ref_jobs[(depth, split)]
    assert r["job_count"].tolist() == [len(w) for w in want]
    assert r["job_first"].tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])[:-1]]).tolist()
    flat = [(i,) + j for i, w in enumerate(want) for j in w]
    assert len(flat) == r["jobs"]
    got = [(int(r["job_root"][j]), _u(r["job_own"][j]), _u(r["job_opp"][j])) + tuple(int(x) for x in r["job_path"][j, :3])
           for j in range(r["jobs"])]
    assert got == flat
    assert not r["job_path"][:, 3].any() and r["job_done"].all()


@pytest.mark.parametrize("depth,split", CASES)
def test_nodes_are_the_expanded_nodes_and_the_jobs_own(split_runs, ref_jobs, depth, split):
    r, want = split_runs[(depth, split)], ref_jobs[(depth, split)]
    flat = [j for w in want for j in w]
    alone = np.zeros(len(flat), dtype=np.int64)
    for d in sorted({j[2] for j in flat}):     # the jobs launched unsplit, a launch per depth
        at = [k for k, j in enumerate(flat) if j[2] == d]
        q = _run([flat[k][0] for k in at], [flat[k][1] for k in at], d)
        assert q["done"].all()
        alone[at] = q["nodes"]
        # a job's score and move are that launch's too
        assert np.array_equal(r["job_score"][at], q["score"]) and np.array_equal(r["job_move"][at], q["move"])
    assert np.array_equal(r["job_nodes"], alone)
    first = 0
    for i, w in enumerate(want):
        assert r["nodes"][i] == sr.expanded_of(w) + alone[first:first + len(w)].sum(), i
        first += len(w)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_batch_shapes(positions, split_runs, n):
    own, opp = positions
    whole = split_runs[(3, 2)]
    idx = [(7 * i + 3) % 49 for i in range(n)]
    r = _run([own[i] for i in idx], [opp[i] for i in idx], 3, split=2)
    assert r["done"].all() and not r["ctl"][[0, 2, 3, 6]].any()
    for k in ("score", "move", "nodes", "job_count"):
        assert np.array_equal(r[k], whole[k][idx]), k
    assert r["jobs"] == whole["job_count"][idx].sum()


def _raw(own, opp, depth, split, capacity, guard=0, count_only=False, fill=0x5A):
    """The C call with the test's own arrays: every job array holds capacity + guard rows filled with `fill` (no job
    arrays at all with count_only).  Returns the return code and the arrays as numpy."""
    n = len(own)
    dev = "cuda"
    t = dict(own=ops.bits_to_tensor(own), opp=ops.bits_to_tensor(opp),
             score=torch.full((n + guard,), fill, dtype=torch.int16, device=dev),
             move=torch.full((n + guard,), fill, dtype=torch.int8, device=dev),
             nodes=torch.full((n + guard,), fill, dtype=torch.int64, device=dev),
             done=torch.full((n + guard,), fill, dtype=torch.uint8, device=dev),
             job_count=torch.full((n + guard,), fill, dtype=torch.int32, device=dev),
             job_first=torch.full((n + guard,), fill, dtype=torch.int64, device=dev),
             ctl=torch.full((8 + guard,), fill, dtype=torch.int32, device=dev))
    a = _lib.AlphaBetaSplitArgs()
    a.n, a.depth, a.split, a.time_limit_ms, a.job_capacity = n, depth, split, 60000, capacity
    if not count_only:
        for k, dt, cols in JOB_ARRAYS:
            t[k] = torch.full(((capacity + guard) * cols,), fill, dtype=dt, device=dev)
    for k, v in t.items():
        if not (count_only and k in ("score", "move", "nodes", "done")):
            setattr(a, k, v.data_ptr())
    rc = _lib.lib().iago_alphabeta_moves_split(C.byref(a), None)
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in t.items()}


def test_count_only(positions, ref_jobs):
    own, opp = positions
    for depth, split in ((3, 1), (4, 2)):
        rc, t = _raw(own, opp, depth, split, 0, guard=4, count_only=True)
        assert rc == 0
        counts = [len(w) for w in ref_jobs[(depth, split)]]
        assert t["job_count"][:49].tolist() == counts
        assert t["job_first"][:49].tolist() == (np.cumsum(counts) - counts).tolist()
        assert t["ctl"][:8].tolist() == [0, 0, 0, 0, sum(counts), 0, 0, 0]
        # nothing else was launched or written
        for k in ("score", "move", "nodes", "done"):
            assert (t[k] == 0x5A).all(), k
        for k in ("job_count", "job_first", "ctl"):
            assert (t[k][-4:] == 0x5A).all(), k


def test_an_exact_capacity_works(positions, split_runs):
    own, opp = positions
    whole = split_runs[(3, 2)]
    r = _run(own, opp, 3, split=2, job_capacity=whole["jobs"])
    assert r["done"].all() and r["ctl"][6] == 0 and r["jobs"] == whole["jobs"]
    for k in ("score", "move", "nodes", "job_own", "job_opp", "job_path", "job_score", "job_nodes"):
        assert np.array_equal(r[k], whole[k]), k
    # and a roomy one: the rows past the jobs are not searched
    r = _run(own, opp, 3, split=2, job_capacity=whole["jobs"] + 1000)
    assert r["done"].all() and r["jobs"] == whole["jobs"]
    for k in ("score", "move", "nodes"):
        assert np.array_equal(r[k], whole[k]), k


def test_a_capacity_one_short_overflows(positions, split_runs):
    own, opp = positions
    whole = split_runs[(3, 2)]
    need = whole["jobs"]
    with pytest.raises(_lib.IagoError, match="job_capacity") as e:
        ops.alphabeta_moves(ops.bits_to_tensor(own), ops.bits_to_tensor(opp), 3, split=2, job_capacity=need - 1)
    assert e.value.jobs_needed == need and str(need) in str(e.value)
    r = _run(own, opp, 3, split=2, job_capacity=need - 1, check_result=False)
    assert r["ctl"][6] != 0 and r["ctl"][4] == need and r["ctl"][5] == 0 and not r["done"].any()
    assert r["ctl"][1] == 0                                   # nothing was claimed: nothing was searched
    guard = 64
    rc, t = _raw(own, opp, 3, 2, need - 1, guard=guard)
    assert rc == 0 and t["ctl"][6] != 0 and t["ctl"][4] == need
    assert not t["done"][:49].any() and t["job_count"][:49].tolist() == whole["job_count"].tolist()
    for k, _, cols in JOB_ARRAYS:
        assert (t[k][(need - 1) * cols:] == 0x5A).all(), k
    for k in ("score", "move", "nodes", "done", "job_count", "job_first", "ctl"):
        assert (t[k][-guard:] == 0x5A).all(), k
    # the same arrays with room for every job: the guard rows stay as they were
    rc, t = _raw(own, opp, 3, 2, need, guard=guard)
    assert rc == 0 and t["ctl"][6] == 0 and t["done"][:49].all()
    assert np.array_equal(t["score"][:49], whole["score"]) and np.array_equal(t["move"][:49], whole["move"])
    for k, _, cols in JOB_ARRAYS:
        assert (t[k][need * cols:] == 0x5A).all(), k
    for k in ("score", "move", "nodes", "done", "job_count", "job_first", "ctl"):
        assert (t[k][-guard:] == 0x5A).all(), k


def test_overlapping_boards_are_refused(positions, split_runs):
    own, opp = positions
    o, p = list(own[:6]), list(opp[:6])
    o[2] |= p[2] & -p[2]          # one stone on both boards
    p[5] |= o[5] & -o[5]
    with pytest.raises(_lib.IagoError, match="refused") as e:
        ops.alphabeta_moves(ops.bits_to_tensor(o), ops.bits_to_tensor(p), 3, split=2)
    assert e.value.result["ctl"][2] == 2
    r = _run(o, p, 3, split=2, check_result=False)
    assert r["ctl"][2] == 2 and r["ctl"][0] == 0 and r["done"].tolist() == [1, 1, 0, 1, 1, 0]
    assert r["job_count"][[2, 5]].tolist() == [0, 0]
    keep = [0, 1, 3, 4]
    for k in ("score", "move", "nodes", "job_count"):
        assert np.array_equal(r[k][keep], split_runs[(3, 2)][k][keep]), k


def test_give_up_on_its_clock():
    own, opp = er.late_positions(256, 61, 30, 44)
    with pytest.raises(_lib.IagoError, match="gave up"):
        ops.alphabeta_moves(ops.bits_to_tensor(own), ops.bits_to_tensor(opp), 10, time_limit_ms=1, split=2)
    r = _run(own, opp, 10, time_limit_ms=1, split=2, check_result=False)
    assert r["ctl"][0] != 0 and not r["done"].all() and r["ctl"][6] == 0
    # what it did finish is what a launch without the limit finds
    fin = np.flatnonzero(r["done"] == 1)
    if len(fin):
        again = _run(own[fin], opp[fin], 10)
        assert np.array_equal(again["score"], r["score"][fin]) and np.array_equal(again["move"], r["move"][fin])
    # a root is done only with all of its jobs
    first, count = r["job_first"], r["job_count"]
    for i in range(256):
        assert r["done"][i] == r["job_done"][first[i]:first[i] + count[i]].all(), i
    # the device is fine afterwards
    s = _run(own[:64], opp[:64], 3, split=2)
    assert s["done"].all() and s["ctl"][0] == 0


def test_split_0_is_the_call_without_the_argument(positions):
    own, opp = positions
    a, b = _run(own, opp, 3), _run(own, opp, 3, split=0, job_capacity=None)
    assert sorted(a) == sorted(b) == ["ctl", "done", "move", "nodes", "score"] and len(a["ctl"]) == 4
    for k in a:
        assert np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype, k


def _match(nets, opponent):  # noqa: F811
    """The paired match of test_match_alphabeta_gpu.py against `opponent`: its records and the turns that overflowed."""
    from iago_amd import engine
    m = engine.BatchedMCTS(B, *nets, lmbda=0.5, c_puct=1.0, n_thr=N_THR, seed=SEED, game_id_base=BASE, persistent=True,
                           capacity=engine.suggest_capacity(N_SIMS, N_THR, moves=64))
    r = engine.SelfPlayEngine(m).play_match(N_SIMS, opponent=opponent, opening_turns=OPENING, paired=True)
    out = {k: getattr(r, k).cpu().numpy() for k in KEYS}
    out.update(n_turns=r.n_turns, launches=r.launches, score=r.score(), split_overflows=r.split_overflows)
    m.close()
    return out


@pytest.fixture(scope="module")
def whole_match(nets):  # noqa: F811
    from iago_amd.engine import AlphaBeta
    return _match(nets, AlphaBeta(3))


@pytest.mark.parametrize("split", [1, 2])
def test_a_match_against_the_split_opponent_is_the_same_match(nets, whole_match, split):  # noqa: F811
    from iago_amd.engine import AlphaBeta
    s = _match(nets, AlphaBeta(3, split=split))
    for k in KEYS:
        assert np.array_equal(s[k], whole_match[k]), k
    assert s["n_turns"] == whole_match["n_turns"] == s["launches"] and s["score"] == whole_match["score"]
    assert (whole_match["valid"] == 2).sum() > B * 20
    assert s["split_overflows"] == whole_match["split_overflows"] == 0


def test_a_match_whose_jobs_never_fit_is_the_same_match(nets, whole_match, monkeypatch):  # noqa: F811
    """A room of one job per game: every turn the opponent moves in overflows and is answered by the unsplit launch."""
    from iago_amd import engine
    monkeypatch.setattr(engine, "ALPHABETA_JOBS_PER_ROOT", {1: 1, 2: 1})
    s = _match(nets, engine.AlphaBeta(3, split=2))
    for k in KEYS:
        assert np.array_equal(s[k], whole_match[k]), k
    assert s["split_overflows"] >= 20 and s["score"] == whole_match["score"]
