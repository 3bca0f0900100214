"""The request rings of the persistent search (tests/ring_util.py: their layout and what a finished launch leaves in
them) after ONE launch of each form, at the small sizes of tests/test_position_table_gpu.py's block b: the single
launch (64 games), the role split (16), the wave search (32 wide, two trees), whole games in one launch (8), a search
whose idle net workgroups walk values ahead (48) and the two-agent arena (8 games a side).  Every other test sees the
rings only through "the trees are bit-identical and nothing gave up"; ring_util.audit looks at the words themselves:
the tails against the request counts, every entry's tags, kind and game, the heads against the tails, the tickets
handed out beyond the tails and the pair walks.

Nothing here breaks the protocol on the device (a dropped ticket makes a launch run to its clock limit);
tests/test_ring_util_cpu.py checks on hand-built rings that the audit does object to each kind of damage."""
import numpy as np
import pytest
import torch

from tests import ring_util as ru
from tests.test_arena_kernel_gpu import _arena, _dev, nets as arena_nets, roots as arena_roots  # noqa: F401  (fixtures)
from tests.test_position_table_gpu import _start, _with_env
from tests.test_search_persistent_gpu import _positions, nets  # noqa: F401  (the fixture: random-initialised nets)
from tests.test_search_wave_gpu import _engine as _wave_engine

pytestmark = pytest.mark.gpu

N_SIMS = 40


def _engine(nets, G, n_sims=N_SIMS, **kw):
    engine, ops, policy, value, rw = nets
    return engine.BatchedMCTS(G, policy, value, rw, n_thr=15, capacity=engine.suggest_capacity(n_sims, 15, moves=2), seed=21,
                              game_id_base=300, persistent=True, **kw)


def _search_once(nets, m, own, opp, n_sims=N_SIMS):
    """ONE launch of m; returns the totals before it."""
    ops = nets[1]
    before = ru.totals_of(m)
    m.search(ops.bits_to_tensor(own), ops.bits_to_tensor(opp), torch.ones(len(own), dtype=torch.uint8, device="cuda"), n_sims)
    torch.cuda.synchronize()
    assert int(m.tree.overflow.sum().item()) == 0
    return before


def _report(form, got):
    print("rings after %s: heads %s, tails %s, tickets beyond the tails %d, pair walks %d, requests of nobody %d" % (
        form, got["heads"], got["tails"], got["beyond"], got["pairs"], got["ahead"]))
    assert got["tails"][ru.KIND_VALUE] > 0 and got["tails"][ru.KIND_POLICY] > 0    # (the launch did use both rings)


def test_single_launch(nets):
    m = _engine(nets, 64)
    before = _search_once(nets, m, *_start(64))
    try:
        assert m._split is None
        _report("the single launch, 64 games", ru.audit(m, before))
    finally:
        m.close()


def test_role_split(nets):
    m = _engine(nets, 16, split=8)
    before = _search_once(nets, m, *_start(16))
    try:
        assert m._split is not None and m.split_cus == 8
        _report("the role split, 16 games", ru.audit(m, before))
    finally:
        m.close()


def test_wave_search(nets):
    m = _wave_engine(nets, 2, N_SIMS, wave=32)
    before = _search_once(nets, m, *_start(2))
    try:
        assert m.wave_entry and m.wave == 32
        _report("the wave search, 32 wide, two trees", ru.audit(m, before))
    finally:
        m.close()


def test_whole_games_in_one_launch(nets):
    engine, ops, policy, value, rw = nets
    m = engine.BatchedMCTS(8, policy, value, rw, n_thr=15, capacity=4096, seed=11, game_id_base=70, persistent=True)
    before = ru.totals_of(m)
    r = engine.SelfPlayEngine(m).play(20)
    try:
        assert r.launches == 1 and r.game_turns is not None
        _report("whole games, 8 in one launch", ru.audit(m, before))
    finally:
        m.close()


def test_values_ahead(nets):
    mp = _with_env({"IAGO_PERSISTENT_AHEAD": "1"})
    try:
        m = _engine(nets, 48)
        before = _search_once(nets, m, *_positions(48))
        try:
            _report("values ahead, 48 games", ru.audit(m, before))
        finally:
            m.close()
    finally:
        mp.undo()


def test_arena(arena_nets, arena_roots):
    ops = arena_nets[1]
    (ma, _), (mb, _) = _arena(arena_nets, _dev(ops, arena_roots, 0, 8), _dev(ops, arena_roots, 8, 16), N_SIMS, N_SIMS)
    try:
        # (a game workgroup of either agent serves both agents' rings once its games are done)
        game_wgs = sum(int(m._ps["ctl"][ru.CTL_FINISHED].item()) for m in (ma, mb))
        zeros = np.zeros(17, np.int64)                       # (fresh engines: _arena builds them)
        for who, m in (("A", ma), ("B", mb)):
            _report("the arena, 8 games a side, agent " + who, ru.audit(m, zeros, game_wgs_serve=game_wgs))
    finally:
        ma.close()
        mb.close()
