"""The wave search (iago_mcts_search_wave, include/iago_hip_serving.h; engine.BatchedMCTS(wave=W)) on the GPU.

  * W = 1 through the new entry point is iago_mcts_search_persistent: every byte of every node, the node counts and
    z_log, also after update_with_move;
  * W = 8 / 32 with vloss 0 / 1 against tests/wave_mcts.py (the oracle's MCTS.py restatement with waves of in-flight
    visits) fed the search's own z_log and the production nets on single boards (NetProbe): visit counts, float32 Q
    and P, child order and the chosen move, bit for bit, on 1 and 4 trees, with a partial last wave, then after
    update_with_move;
  * the trees do not depend on the net workgroups' number or the position table; a finished search leaves every
    in-flight count (vv) at 0;
  * refusals; the front end (MCTS(wave=32), an --auto game.Game).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import mcts_py
from oracle import oracle as orc
from tests.conftest import GOLDEN, load_json
from tests.gpu_util import state_of
from tests.test_mcts_production_gpu import NetProbe, _positions
from tests.test_oracle_golden import _cmp_tree
from tests.wave_mcts import WaveMCTS

pytestmark = pytest.mark.gpu

START_OWN, START_OPP = 0x0000000810000000, 0x0000001008000000


@pytest.fixture(scope="module")
def shipped():
    from iago_amd import engine, network, ops
    assert torch.cuda.is_available()
    policy = network.SLPolicy().load_npz(os.path.join(GOLDEN, "sl_model.npz")).cuda().eval()
    value = network.Value().load_npz(os.path.join(GOLDEN, "value_model.npz")).cuda().eval()
    g = load_json("simulate.json")
    return engine, ops, policy, value, ops.RolloutWeights(g["shipped_w"], g["shipped_b"])


def _engine(shipped, G, n_sims, wave=1, vloss=1.0, **kw):
    engine, ops, policy, value, rw = shipped
    cap = engine.suggest_capacity(n_sims + 60, 15, moves=2)
    m = engine.BatchedMCTS(G, policy, value, rw, lmbda=0.5, c_puct=1.0, n_thr=15, capacity=cap, seed=5,
                           game_id_base=1000, z_log_rows=max(n_sims, 60), wave=wave, virtual_loss=vloss, **kw)
    assert m.persistent and m.wave == wave and m.wave_entry == (wave > 1)
    return m


def _vv(m):
    return m.tree.nodes.view(-1, 8)[:, 7]


def _two_searches(m, own, opp, active, n_sims, n_sims2=60):
    """A search, the most visited moves, update_with_move, a search of the other side; the host copies along the way."""
    from iago_amd import ops
    o, p = ops.bits_to_tensor(own), ops.bits_to_tensor(opp)
    m.search(o, p, active, n_sims)
    torch.cuda.synchronize()
    first = dict(move=m.best_move(active)[0].cpu().numpy().copy(), visits=m.visits.cpu().numpy().copy(),
                 zlog=m.z_log.cpu().numpy().copy(), zn=m.z_log_n.cpu().numpy().copy(),
                 nodes=m.tree.nodes.cpu().clone(), n_nodes=m.tree.n_nodes.cpu().clone())
    mv = torch.from_numpy(np.where(first["move"] == -2, -1, first["move"]).astype(np.int8)).cuda()
    m.update_with_move(mv, active.clone())
    o2, p2 = o.clone(), p.clone()
    ops.apply_moves(o2, p2, mv)
    m.z_log_n.zero_()
    m.search(p2, o2, active, n_sims2)
    torch.cuda.synchronize()
    second = dict(zlog=m.z_log.cpu().numpy().copy(), zn=m.z_log_n.cpu().numpy().copy(),
                  nodes=m.tree.nodes.cpu().clone(), n_nodes=m.tree.n_nodes.cpu().clone())
    return first, second, mv.cpu().numpy()


def test_wave_one_is_the_persistent_search(shipped, golden_rules):
    """Test 1: W = 1 through iago_mcts_search_wave == iago_mcts_search_persistent, all 32 bytes of every node."""
    G, n_sims = 64, 100
    own, opp = _positions(G, golden_rules)
    active = torch.ones(G, dtype=torch.uint8, device="cuda")
    active[5] = 0
    ref = _engine(shipped, G, n_sims)
    got = _engine(shipped, G, n_sims)
    got.wave_entry = True
    r1, r2, _ = _two_searches(ref, own, opp, active, n_sims)
    g1, g2, _ = _two_searches(got, own, opp, active, n_sims)
    for a, b in ((r1, g1), (r2, g2)):
        assert torch.equal(a["n_nodes"], b["n_nodes"])
        assert torch.equal(a["nodes"], b["nodes"])
        assert np.array_equal(a["zlog"], b["zlog"]) and np.array_equal(a["zn"], b["zn"])
    assert int(_vv(got).abs().sum().item()) == 0


def _oracle_check(shipped, m, own, opp, first, second, mv, trees, n_sims, n_sims2, wave, vloss):
    engine, ops, policy, value, rw = shipped
    probe = NetProbe(ops, policy, value)
    for g in trees:
        it = iter(first["zlog"][:n_sims, g])
        om = WaveMCTS(probe.policy_fn, probe.value_fn, lambda s, c, it=it: int(next(it)), lmbda=0.5, c_puct=1.0,
                      n_thr=15, wave=wave, vloss=vloss)
        want = om.get_move(state_of(own[g], opp[g]), 1, n_sims)
        assert next(it, None) is None
        assert first["move"][g] == (-2 if want is None else want), g
        for a, ch in om.root.children.items():
            if a >= 0:
                assert first["visits"][g, a] == ch.n_visits
        a = int(mv[g])
        om.update_with_move(a)
        s = state_of(own[g], opp[g])
        orc.place_stone(s, a, 1)
        it = iter(second["zlog"][:n_sims2, g])
        om.rollout_fn = lambda st, c, it=it: int(next(it))
        om.get_move(s, 2, n_sims2)
        assert next(it, None) is None
        _cmp_tree(m.tree.dump(g, max_depth=64), mcts_py.dump_tree(om.root, max_depth=64), "g%d W%d" % (g, wave))


@pytest.mark.parametrize("wave,vloss,G,n_sims", [(8, 1.0, 4, 100), (32, 1.0, 1, 100), (32, 0.0, 4, 37),
                                                 (8, 0.0, 1, 37), (32, 1.0, 4, 37)])
def test_wave_trees_vs_restatement(shipped, golden_rules, wave, vloss, G, n_sims):
    """Test 2 (and 4): the trees of the wave search are the restatement's, bit for bit; vv is 0 afterwards."""
    own, opp = _positions(8, golden_rules)
    own, opp = own[:G].copy(), opp[:G].copy()
    own[0], opp[0] = START_OWN, START_OPP
    m = _engine(shipped, G, n_sims, wave=wave, vloss=vloss)
    active = torch.ones(G, dtype=torch.uint8, device="cuda")
    first, second, mv = _two_searches(m, own, opp, active, n_sims)
    assert np.all(first["zn"] == n_sims) and np.all(second["zn"] == 60)
    assert int(_vv(m).abs().sum().item()) == 0
    _oracle_check(shipped, m, own, opp, first, second, mv, range(G), n_sims, 60, wave, vloss)


def test_wave_trees_do_not_depend_on_nets_or_table(shipped, golden_rules, monkeypatch):
    """Test 3: 8 net workgroups against the default, the position table off against on -- the same trees."""
    G, n_sims = 4, 100
    own, opp = _positions(8, golden_rules)
    own, opp = own[:G].copy(), opp[:G].copy()
    active = torch.ones(G, dtype=torch.uint8, device="cuda")
    runs = []
    for kw, table in (({}, None), ({"net_workgroups": 8}, None), ({}, "0")):
        if table is not None:
            monkeypatch.setenv("IAGO_PERSISTENT_TABLE", table)
        m = _engine(shipped, G, n_sims, wave=32, **kw)
        assert (m._vtable is None) == (table == "0")
        first, second, _ = _two_searches(m, own, opp, active, n_sims)
        runs.append((first, second))
    for f, s in runs[1:]:
        for a, b in ((runs[0][0], f), (runs[0][1], s)):
            assert torch.equal(a["nodes"], b["nodes"]) and torch.equal(a["n_nodes"], b["n_nodes"])
            assert np.array_equal(a["zlog"], b["zlog"])


def test_wave_refusals(shipped):
    """Test 5: bad widths and whole games through the C ABI, bad options in the engine."""
    from iago_amd import _lib
    L = _lib.lib()
    a = _lib.MctsSearchArgs()
    for width, vloss, max_turns in ((4, 1.0, 0), (0, 1.0, 0), (64, 1.0, 0), (8, -1.0, 0), (8, float("nan"), 0),
                                    (8, 1.0, 10), (1, 1.0, 1)):
        w = _lib.SearchWaveArgs()
        w.width, w.vloss = width, vloss
        a.max_turns = max_turns
        assert L.iago_mcts_search_wave(C.byref(a), C.byref(w), None) == -1   # IAGO_ERR_INVALID
    for bad in (4, 0, 2, True, 64):
        with pytest.raises(ValueError):
            _engine(shipped, 1, 100, wave=bad)
    with pytest.raises(ValueError):
        _engine(shipped, 1, 100, wave=8, vloss=-1.0)


def test_front_end_wave(shipped):
    """Test 6: MCTS(wave=32, n_sims=200).get_move from the start position is the restatement's move (through the
    engine it wraps, whose z_log feeds the restatement), and an --auto game.Game with wave=32 plays to the end."""
    engine, ops, policy, value, rw = shipped
    from iago_amd.MCTS import MCTS
    from iago_amd.game import Game
    mc = MCTS(policy_net=policy, value_net=value, rollout_weights=rw, n_sims=200, wave=32, seed=3, capacity=8192)
    move = mc.get_move(orc.initial_state(), 1)
    m = engine.BatchedMCTS(1, policy, value, rw, lmbda=0.5, c_puct=1, n_thr=15, capacity=8192, seed=3, z_log_rows=200,
                           wave=32)
    one = torch.ones(1, dtype=torch.uint8, device="cuda")
    m.search(ops.bits_to_tensor([START_OWN]), ops.bits_to_tensor([START_OPP]), one, 200)
    assert int(m.best_move(one)[0].item()) == move
    probe = NetProbe(ops, policy, value)
    it = iter(m.z_log.cpu().numpy()[:200, 0])
    om = WaveMCTS(probe.policy_fn, probe.value_fn, lambda s, c: int(next(it)), lmbda=0.5, c_puct=1, n_thr=15, wave=32)
    assert om.get_move(orc.initial_state(), 1, 200) == move
    _cmp_tree(mc._m.tree.dump(0, max_depth=64), mcts_py.dump_tree(om.root, max_depth=64), "front end")

    mc2 = MCTS(policy_net=policy, value_net=value, rollout_weights=rw, n_sims=40, wave=32, seed=4, capacity=65536)
    lines = []
    g = Game(True, model=policy, mcts=mc2, date="2000-01-01-00-00", out=lines.append)
    from iago_amd import game as game_mod
    jd = game_mod.play(g, True)
    assert g.stone_num >= 64 and jd and jd in lines
