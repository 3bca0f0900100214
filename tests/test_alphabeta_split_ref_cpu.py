"""The root split of the alpha-beta opponent without a GPU: the restatement (tests/alphabeta_split_ref.py) against the
plain minimax, the kinds of job its position set holds, the ABI entry and every refusal that needs no device."""
import ctypes as C
import os
import re

import pytest

from . import alphabeta_ref as ab
from . import alphabeta_split_ref as sr
from . import endgame_ref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def positions():
    return sr.position_set()


@pytest.mark.parametrize("depth,split", [(2, 1), (3, 1), (3, 2)])
def test_the_jobs_combine_to_the_minimax(positions, depth, split):
    own, opp = positions
    assert len(own) == 49
    for i, (a, b) in enumerate(zip(own, opp)):
        assert sr.split_minimax(a, b, depth, split) == ab.minimax(a, b, depth), i


def test_the_position_set_holds_every_kind_of_job(positions):
    own, opp = positions
    per_root = [sr.jobs_of(a, b, 3, 2) for a, b in zip(own[:48], opp[:48])]
    jobs = [j for r in per_root for j in r]
    assert len(jobs) == 2308 and len(jobs) % 64 != 0
    assert sr.job_kinds(jobs) == (10, 7, 2291)
    assert max(len(r) for r in per_root) == 180
    assert sum(len(sr.jobs_of(a, b, 3, 1)) for a, b in zip(own[:48], opp[:48])) == 266
    # the depths: a root that is its own job keeps the full depth, a child that cannot move depth - 1
    for d, s in ((3, 2), (6, 2), (4, 1)):
        for a, b, left, m1, m2 in (j for x, y in zip(own, opp) for j in sr.jobs_of(x, y, d, s)):
            assert left == (d if m1 < 0 else d - 1 if m2 < 0 else d - 2)
            assert left >= 1 and (m2 < 0 or s == 2)
    # canonical order
    for r in per_root:
        assert [(j[3], j[4]) for j in r] == sorted((j[3], j[4]) for j in r)
    assert [sr.expanded_of(r) for r in per_root].count(0) == 10


def test_a_child_that_must_pass_while_the_game_goes_on(positions):
    own, opp = positions
    # none among the first 48: their one-ply jobs at split 2 are finished games
    for a, b in zip(own[:48], opp[:48]):
        for x, y, _, m1, m2 in sr.jobs_of(a, b, 3, 2):
            if m1 >= 0 and m2 < 0:
                assert not er.bit_legal(x, y) and not er.bit_legal(y, x)
    a, b = sr.child_must_pass()
    assert (a, b) == (own[48], opp[48])
    jobs = sr.jobs_of(a, b, 3, 2)
    kind = [j for j in jobs if j[3] == 47 and j[4] < 0]
    assert len(kind) == 1
    x, y, left, _, _ = kind[0]
    assert not er.bit_legal(x, y) and er.bit_legal(y, x) and left == 2
    assert any(j[4] >= 0 for j in jobs)                      # beside expanded children
    assert sr.expanded_of(jobs) == 1 + len({j[3] for j in jobs if j[4] >= 0})


def test_the_restatement_refuses_bad_splits():
    for depth, split in ((3, 0), (3, 3), (2, 2), (1, 1), (4, -1)):
        with pytest.raises(ValueError, match="split"):
            sr.jobs_of(1, 2, depth, split)


def test_serving_header_lists_the_split():
    from iago_amd import _lib
    text = open(os.path.join(ROOT, "include", "iago_hip_serving.h")).read()
    declared = set(re.findall(r"IAGO_API[^;(]*?\b(iago_\w+)\s*\(", text))
    L = _lib.lib()
    name = "iago_alphabeta_moves_split"
    assert name in declared and name in _lib.SERVING_SYMBOLS and hasattr(L, name)
    assert "typedef struct iago_alphabeta_split_args" in text
    # 2 pointers and n; depth, split, time_limit_ms, reserved0; 4 results; job_count, job_first, job_capacity; 8 job
    # arrays; ctl; reserved[4]
    assert C.sizeof(_lib.AlphaBetaSplitArgs) == 8 * 3 + 4 * 4 + 8 * 4 + 8 * 3 + 8 * 8 + 8 + 8 * 4 == 200
    assert _lib.AlphaBetaSplitArgs._fields_[-1][0] == "reserved" and _lib.AlphaBetaSplitArgs.reserved.size == 32
    assert _lib.AlphaBetaSplitArgs.reserved.offset == 200 - 32
    assert re.search(r"#define\s+IAGO_ALPHABETA_MAX_SPLIT\s+2\b", text) and _lib.ALPHABETA_MAX_SPLIT == 2
    assert re.search(r"#define\s+IAGO_ALPHABETA_SPLIT_CTL_WORDS\s+8\b", text) and _lib.ALPHABETA_SPLIT_CTL_WORDS == 8
    # the unsplit entry point is as it was
    assert C.sizeof(_lib.AlphaBetaArgs) == 8 * 3 + 4 * 2 + 8 * 5 + 8 * 4 and L.iago_abi_version() == 13


JOB_ARRAYS = ("job_own", "job_opp", "job_root", "job_path", "job_score", "job_move", "job_nodes", "job_done")


def test_host_side_refusals():
    from iago_amd import _lib
    L = _lib.lib()
    buf = (C.c_uint64 * 8)()
    ctl = (C.c_uint32 * 8)()

    def args(**kw):
        a = _lib.AlphaBetaSplitArgs()
        for f in ("own", "opp", "score", "move", "nodes", "done", "job_count", "job_first") + JOB_ARRAYS:
            setattr(a, f, C.addressof(buf))
        a.ctl = C.addressof(ctl)
        a.n, a.depth, a.split, a.time_limit_ms, a.job_capacity = 1, 4, 2, 1000, 1
        for k, v in kw.items():
            if k == "reserved":
                a.reserved[2] = v
            else:
                setattr(a, k, v)
        return a

    assert L.iago_alphabeta_moves_split(None, None) == _lib.IAGO_ERR_INVALID
    cases = [dict(own=None), dict(opp=None), dict(score=None), dict(move=None), dict(nodes=None), dict(done=None),
             dict(job_count=None), dict(job_first=None), dict(ctl=None), dict(n=-1), dict(n=2 ** 31),
             dict(split=0), dict(split=3), dict(split=-1), dict(depth=2, split=2), dict(depth=1, split=1),
             dict(depth=3, split=3), dict(depth=11), dict(depth=0), dict(time_limit_ms=0), dict(time_limit_ms=600001),
             dict(job_capacity=-1), dict(job_capacity=2 ** 31), dict(reserved=7), dict(reserved0=1)]
    cases += [{k: None} for k in JOB_ARRAYS]                        # some job arrays but not all
    cases += [dict({k: None for k in JOB_ARRAYS}, job_capacity=1)]  # no job arrays, but room asked for
    for kw in cases:
        assert L.iago_alphabeta_moves_split(C.byref(args(**kw)), None) == _lib.IAGO_ERR_INVALID, kw
        assert b"iago_alphabeta_moves_split" in L.iago_last_error()


def test_python_entry_points_refuse_bad_options():
    import torch
    from iago_amd import _lib, engine, ops
    t = torch.zeros(2, dtype=torch.int64)
    for depth, bad in ((4, 3), (4, -1), (4, 1.0), (4, True), (4, "1"), (4, None), (2, 2), (1, 1), (3, 3)):
        with pytest.raises(ValueError, match="split"):
            ops.alphabeta_moves(t, t, depth, split=bad)
        with pytest.raises(ValueError, match="split"):
            engine.AlphaBeta(depth, split=bad)
        with pytest.raises(ValueError, match="split"):
            engine.AlphaBeta(depth, bad)
    for bad in (-1, 1.5, True, "9", 2 ** 31):
        with pytest.raises(ValueError, match="job_capacity"):
            ops.alphabeta_moves(t, t, 4, split=1, job_capacity=bad)
    with pytest.raises(ValueError):
        ops.alphabeta_moves(t, t[:1], 4, split=1)
    for cap in (None, 8):
        with pytest.raises(_lib.IagoError):
            ops.alphabeta_moves(t, t, 4, split=2, job_capacity=cap)       # CPU tensors: no CPU fallback
    assert engine.AlphaBeta(3) == engine.AlphaBeta(3, split=0) == engine.AlphaBeta(3, 0) == (3, 0)
    assert engine.AlphaBeta(3).split == 0 and engine.AlphaBeta(6, split=2).split == 2
    assert engine.AlphaBeta(3, split=1) != engine.AlphaBeta(3)
    assert engine.AlphaBeta._fields == ("depth", "split")
    assert engine.ALPHABETA_JOBS_PER_ROOT == {1: 32, 2: 1024}
    assert ops.alphabeta_job_count([0, 0, 0, 0, 5, 1, 0, 0]) == 5 + 2 ** 32
    assert ops.alphabeta_job_count([0, 0, 0, 0, -1, 0, 0, 0]) == 2 ** 32 - 1     # (ctl is read as int32)


class _StubMcts(object):
    """What SelfPlayEngine reads before its first device call; anything else is a failure of the test."""
    n_games = 4

    def __getattr__(self, name):
        raise AssertionError("play_match must check its arguments before the engine is touched (read %r)" % name)


def test_play_match_refusals_before_the_device():
    from iago_amd.engine import AlphaBeta, SelfPlayEngine
    e = SelfPlayEngine(_StubMcts())
    for bad in (AlphaBeta._make((3, 3)), AlphaBeta._make((2, 2)), AlphaBeta(4)._replace(split=-1),
                AlphaBeta(4)._replace(split=True), AlphaBeta._make((1, 1))):
        with pytest.raises(ValueError, match="split"):
            e.play_match(24, opponent=bad)
    with pytest.raises(ValueError, match="depth"):
        e.play_match(24, opponent=AlphaBeta._make((11, 1)))
    with pytest.raises(ValueError, match="opening_turns"):
        e.play_match(24, opponent=AlphaBeta(3, split=2), opening_turns=3)
