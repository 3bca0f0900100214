"""The root split of the exact solver without a GPU: the restatement (tests/endgame_split_ref.py) against the plain
negamax and the restated root rules BEST / ALL, the kinds of job its position set holds, the ABI entry and every refusal
that needs no device."""
import ctypes as C
import os
import re

import pytest

from . import endgame_moves_ref as mr
from . import endgame_ref as er
from . import endgame_split_ref as sr
from . import lane_search_ref as ls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def positions():
    own, opp = sr.position_set()
    assert len(own) == 54 and max(er.empties(a, b) for a, b in zip(own, opp)) == 8
    return own, opp


@pytest.mark.parametrize("wld", [False, True])
@pytest.mark.parametrize("split", [1, 2])
def test_the_jobs_combine_to_the_solvers_answers(positions, split, wld):
    own, opp = positions
    for i, (a, b) in enumerate(zip(own, opp)):
        r = sr.split_solve(a, b, split, wld)
        assert (r["score"], r["move"]) == er.solve_bits(a, b, wld=wld), i
        score, move, _, best, scores = mr.solve_moves(a, b, wld, mr.ALL)
        assert (r["score"], r["move"], r["best"]) == (score, move, best), i
        assert r["row"] == [scores.get(m, sr.NO_MOVE) for m in range(64)], i
        assert best == mr.solve_moves(a, b, wld, mr.BEST)[3], i
        # the node rule: the nodes expanded and the jobs' own, each job lane_search_ref's
        assert r["nodes"] == sr.expanded_of(r["jobs"]) + sum(ls.solve(j[0], j[1], wld)[2] for j in r["jobs"])
        assert r["job_values"] == [ls.solve(j[0], j[1], wld) for j in r["jobs"]]


def test_the_position_set_holds_every_kind_of_job(positions):
    own, opp = positions
    kinds = [sr.kinds_of(a, b) for a, b in zip(own, opp)]
    assert set().union(*kinds) == sr.KINDS
    by_name = {name: (a, b) for name, a, b in mr.hand_made()}
    at = {name: kinds[own.index(a)] for name, (a, b) in by_name.items()}
    assert "root_pass" in at["one_pass"] and "root_over" in at["full"] and "root_over" in at["dead"]
    assert at["full"] >= {"empties0"} and at["one"] >= {"empties1", "child_over"} and at["two"] >= {"empties2", "tie"}
    assert "child_pass" in kinds[-1] and "two_ply" in kinds[-1] and (own[-1], opp[-1]) == sr.child_must_pass()
    # the child that must pass: its mover has no move, the other side has one, the game goes on
    a, b, left, m1, m2 = [j for j in sr.jobs_of(own[-1], opp[-1], 2) if j[3] >= 0 and j[4] < 0][0]
    assert not er.bit_legal(a, b) and er.bit_legal(b, a) and left == er.empties(own[-1], opp[-1]) - 1
    for split in (1, 2):
        per_root = [sr.jobs_of(a, b, split) for a, b in zip(own, opp)]
        for (a, b), r in zip(zip(own, opp), per_root):
            assert [(j[3], j[4]) for j in r] == sorted((j[3], j[4]) for j in r)     # canonical order
            e = er.empties(a, b)
            for x, y, left, m1, m2 in r:
                assert left == er.empties(x, y) == e - (m1 >= 0) - (m2 >= 0) and (m2 < 0 or split == 2)
        assert sum(len(r) for r in per_root) % 64 != 0
        # roots with fewer empties than split plies end in finished-game jobs
        for (a, b), r in zip(zip(own, opp), per_root):
            if er.empties(a, b) < split and r[0][3] >= 0:
                assert all(not er.bit_legal(x, y) and not er.bit_legal(y, x) for x, y, _, _, _ in r)


def test_the_restatement_refuses_bad_splits():
    for split in (0, 3, -1, True, None):
        with pytest.raises(ValueError, match="split"):
            sr.jobs_of(1, 2, split)


def test_serving_header_lists_the_split():
    from iago_amd import _lib
    text = open(os.path.join(ROOT, "include", "iago_hip_serving.h")).read()
    declared = set(re.findall(r"IAGO_API[^;(]*?\b(iago_\w+)\s*\(", text))
    L = _lib.lib()
    name = "iago_solve_endgame_split"
    assert name in declared and name in _lib.SERVING_SYMBOLS and hasattr(L, name)
    assert "typedef struct iago_endgame_split_args" in text
    # 2 pointers and n; mode, split, max_empties, time_limit_ms; 4 results and the 2 optional ones; job_count,
    # job_first, job_capacity; 8 job arrays; ctl; reserved[4]
    assert C.sizeof(_lib.EndgameSplitArgs) == 8 * 3 + 4 * 4 + 8 * 6 + 8 * 3 + 8 * 8 + 8 + 8 * 4 == 216
    assert _lib.EndgameSplitArgs._fields_[-1][0] == "reserved" and _lib.EndgameSplitArgs.reserved.offset == 216 - 32
    assert re.search(r"#define\s+IAGO_ENDGAME_MAX_SPLIT\s+2\b", text) and _lib.ENDGAME_MAX_SPLIT == 2
    assert re.search(r"#define\s+IAGO_ENDGAME_SPLIT_CTL_WORDS\s+8\b", text) and _lib.ENDGAME_SPLIT_CTL_WORDS == 8
    # the unsplit entry points and the version are as they were
    assert C.sizeof(_lib.EndgameArgs) == 8 * 3 + 4 * 4 + 8 * 5 + 8 * 4 and L.iago_abi_version() == 13


JOB_ARRAYS = ("job_own", "job_opp", "job_root", "job_path", "job_score", "job_move", "job_nodes", "job_done")


def test_host_side_refusals():
    from iago_amd import _lib
    L = _lib.lib()
    buf = (C.c_uint64 * 64)()
    ctl = (C.c_uint32 * 8)()

    def args(**kw):
        a = _lib.EndgameSplitArgs()
        for f in ("own", "opp", "score", "move", "nodes", "solved", "best", "move_score", "job_count",
                  "job_first") + JOB_ARRAYS:
            setattr(a, f, C.addressof(buf))
        a.ctl = C.addressof(ctl)
        a.n, a.mode, a.split, a.max_empties, a.time_limit_ms, a.job_capacity = 1, 0, 2, 10, 1000, 1
        for k, v in kw.items():
            if k == "reserved":
                a.reserved[2] = v
            else:
                setattr(a, k, v)
        return a

    assert L.iago_solve_endgame_split(None, None) == _lib.IAGO_ERR_INVALID
    assert b"iago_solve_endgame_split" in L.iago_last_error()
    cases = [dict(own=None), dict(opp=None), dict(score=None), dict(move=None), dict(nodes=None), dict(solved=None),
             dict(job_count=None), dict(job_first=None), dict(ctl=None), dict(n=-1), dict(n=2 ** 31),
             dict(split=0), dict(split=3), dict(split=-1), dict(mode=2), dict(mode=-1), dict(max_empties=-1),
             dict(max_empties=21), dict(time_limit_ms=0), dict(time_limit_ms=600001),
             dict(job_capacity=-1), dict(job_capacity=2 ** 31), dict(reserved=7)]
    cases += [{k: None} for k in JOB_ARRAYS]                        # some job arrays but not all
    cases += [dict({k: None for k in JOB_ARRAYS}, job_capacity=1)]  # no job arrays, but room asked for
    for kw in cases:
        assert L.iago_solve_endgame_split(C.byref(args(**kw)), None) == _lib.IAGO_ERR_INVALID, kw
        assert b"iago_solve_endgame_split" in L.iago_last_error(), kw


def test_python_entry_points_refuse_bad_options():
    import inspect

    import torch
    from iago_amd import _lib, engine, ops, value_self_play
    t = torch.zeros(2, dtype=torch.int64)
    for bad in (3, -1, 1.0, True, "1", None):
        with pytest.raises(ValueError, match="split"):
            ops.solve_endgame(t, t, split=bad)
        with pytest.raises(ValueError, match="split"):
            ops.solve_endgame_moves(t, t, moves="all", split=bad)
        with pytest.raises(ValueError, match="split"):
            value_self_play.generate(None, None, 1, exact_empties=4, exact_split=bad)
    for bad in (-1, 1.5, True, "9", 2 ** 31):
        with pytest.raises(ValueError, match="job_capacity"):
            ops.solve_endgame(t, t, split=1, job_capacity=bad)
    with pytest.raises(ValueError):
        ops.solve_endgame(t, t[:1], split=1)
    for cap in (None, 8):
        with pytest.raises(_lib.IagoError):
            ops.solve_endgame(t, t, split=2, job_capacity=cap)        # CPU tensors: no CPU fallback
    # the defaults stay unsplit
    for f, name in ((ops.solve_endgame, "split"), (ops.solve_endgame_moves, "split"), (engine.endgame_errors, "split"),
                    (value_self_play.generate, "exact_split")):
        assert inspect.signature(f).parameters[name].default == 0
