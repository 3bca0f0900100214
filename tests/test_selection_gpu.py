"""The AlphaZero selection rule of the persistent search (engine.BatchedMCTS(selection="alphazero"); IAGO_SEARCH_PUCT_AZ in
include/iago_hip_serving.h; csrc/mcts_dev.hpp "the selection rule", csrc/search_kernel.hip SearchParams.prior_off /
visit_off) against its restatement (tests/selection_ref.py: a child stores float32(prob), the exploration term divides by
1 + n), bit for bit, in every form that creates children or scores them: single searches with subtree reuse at n_thr 15
and 1, alone and together with the negamax backup; whole games in one launch / through the turn loop / as a stream, the
role split; the wave search; an arena of an "alphazero" agent against a "reference" agent; and composed with exploring
openings, the playout cap, the exact endgame, root noise, forced playouts and their pruning.  selection="reference" is the
engine of before, dump for dump.  Every reference is fed the search's own z_log and the production nets on one board
(NetProbe).  Sizes are test_negamax_gpu.py's or smaller; tests/test_selection_ref_cpu.py shows that the rules differ there."""
import os
import types

import numpy as np
import pytest
import torch

from oracle import mcts_py
from oracle import oracle as orc
from tests import negamax_ref, selection_ref
from tests.conftest import GOLDEN, load_json
from tests.gpu_util import state_of
from tests.test_mcts_production_gpu import NetProbe, _positions
from tests.test_negamax_gpu import RECORDS, _reference_check, _same, _two_searches

pytestmark = pytest.mark.gpu

N_SIMS = 20


@pytest.fixture(scope="module")
def shipped():
    from iago_amd import engine, network, ops
    assert torch.cuda.is_available()
    policy = network.SLPolicy().load_npz(os.path.join(GOLDEN, "sl_model.npz")).cuda().eval()
    value = network.Value().load_npz(os.path.join(GOLDEN, "value_model.npz")).cuda().eval()
    g = load_json("simulate.json")
    return engine, ops, policy, value, ops.RolloutWeights(g["shipped_w"], g["shipped_b"])


@pytest.fixture(scope="module")
def probe(shipped):
    return NetProbe(shipped[1], shipped[2], shipped[3])     # (memoised: the module's references share the nets' answers)


def _priors_exact(got, want, path="root"):
    """_cmp_tree allows the reference's float64 1.1 of a lone child one part in 1e7; under the rule every stored prior of a
    node below the root is a float32 on both sides: the same bits."""
    for a in want["children"]:
        g, w = got["children"][a], want["children"][a]
        assert np.float32(g["P"]).tobytes() == np.float32(w["P"]).tobytes(), (path, a, g["P"], w["P"])
        _priors_exact(g, w, path + "/" + a)


# ---- 1. / 2. trees: two searches with update_with_move between them
CHECKED = [0, 1, 2, 3, 4, 12, 13, 14, 15, 16]


@pytest.fixture(scope="module")
def parent_dumps(shipped, golden_rules):
    """The engine without the argument, per n_thr: computed once, shared by the tests that compare against it."""
    own, opp = _positions(24, golden_rules)
    return {n_thr: _two_searches(shipped, own, opp, n_thr) for n_thr in (15, 1)}


@pytest.mark.parametrize("n_thr", [15, 1])
def test_trees_bit_exact_vs_the_restatement(shipped, probe, golden_rules, parent_dumps, n_thr):
    """24 games -- start positions, midgames, 'pass1' / 'dead' / 'full' at 1 / 2 / 3 --, 100 playouts, update_with_move, 37
    more from the other side.  Ten games against the restatement; selection="reference" is the engine without the
    argument, dump for dump, and the flag is set only where asked."""
    from iago_amd import _lib
    own, opp = _positions(24, golden_rules)
    az = _two_searches(shipped, own, opp, n_thr, selection="alphazero")
    ref = _two_searches(shipped, own, opp, n_thr, selection="reference")
    old = parent_dumps[n_thr]
    assert az["flag"] & _lib.SEARCH_PUCT_AZ and not (ref["flag"] | old["flag"]) & _lib.SEARCH_PUCT_AZ
    assert not (az["flag"] | ref["flag"] | old["flag"]) & _lib.SEARCH_NEGAMAX
    for k in ("first", "second"):
        assert ref[k] == old[k], k                        # dump for dump, every game
    assert np.array_equal(ref["move"], old["move"]) and np.array_equal(ref["z1"], old["z1"])
    with selection_ref.rule():
        _reference_check(probe, az, own, opp, CHECKED, n_thr)
        for g in CHECKED:                                  # (the first search's stored priors, to the bit)
            om = mcts_py.MCTS(probe.policy_fn, probe.value_fn, lambda s, c, it=iter(az["z1"][:100, g]): int(next(it)),
                              lmbda=0.5, c_puct=1.0, n_thr=n_thr)
            om.get_move(state_of(own[g], opp[g]), 1, 100)
            _priors_exact(az["first"][g], mcts_py.dump_tree(om.root, max_depth=64), "g%d" % g)
    _reference_check(probe, old, own, opp, CHECKED[:2] + CHECKED[5:7], n_thr)   # (and the default is the oracle's own rule)
    differ = [g for g in CHECKED if az["second"][g] != ref["second"][g]]
    moved = int(np.sum(az["move"] != ref["move"]))
    print("n_thr %d: %d of %d checked trees differ from the reference rule's, %d of 24 moves" % (n_thr, len(differ),
                                                                                                len(CHECKED), moved))
    assert differ
    # a fresh root's 1.1 under both rules; the lone (pass) child of the dead board: 1.0 under the rule
    assert az["first"][2]["P"] == ref["first"][2]["P"] == float(np.float32(np.float32(1.0) + np.float32(0.1)))
    assert az["first"][2]["order"] == [-1] and az["first"][2]["children"]["-1"]["P"] == 1.0
    assert ref["first"][2]["children"]["-1"]["P"] == az["first"][2]["P"]


@pytest.mark.parametrize("n_thr", [15, 1])
def test_both_rules_together(shipped, probe, golden_rules, n_thr):
    from iago_amd import _lib
    own, opp = _positions(24, golden_rules)
    both = _two_searches(shipped, own, opp, n_thr, selection="alphazero", backup="negamax")
    assert both["flag"] & _lib.SEARCH_PUCT_AZ and both["flag"] & _lib.SEARCH_NEGAMAX
    with selection_ref.rule(), negamax_ref.rule():
        _reference_check(probe, both, own, opp, CHECKED, n_thr)


# ---- 3. whole games
def _play(shipped, G=8, n_sims=N_SIMS, how="play", base=70, z_log=True, n_thr=15, engine_kw=None, selection="alphazero", **kw):
    engine, ops, policy, value, rw = shipped
    m = engine.BatchedMCTS(G, policy, value, rw, n_thr=n_thr, capacity=4096, seed=11, game_id_base=base, persistent=True,
                           selection=selection, **(dict(z_log_rows=128 * n_sims) if z_log else {}), **(engine_kw or {}))
    e = engine.SelfPlayEngine(m)
    r = e.play(n_sims, **kw) if how == "play" else e.play_stream(n_sims, how, **kw)
    out = {k: getattr(r, k).cpu().numpy() for k in RECORDS}
    out["game_turns"] = r.game_turns.cpu().numpy() if r.game_turns is not None else None
    out.update(n_turns=r.n_turns, launches=r.launches, replayed=e.n_replayed, split=m._split is not None,
               gave_up=int(m._ps["ctl"][3].item()), overflow=int(m.tree.overflow.sum().item()))
    if z_log:
        out["zlog"], out["zn"] = m.z_log.cpu().numpy().copy(), m.z_log_n.cpu().numpy().copy()
    m.close()
    assert out["gave_up"] == 0 and out["overflow"] == 0
    return out


@pytest.fixture(scope="module")
def one_launch_games(shipped):
    out = _play(shipped)
    assert out["launches"] == 1 and out["replayed"] == 0
    return out


def test_whole_games_one_launch_turn_loop_and_restatement(shipped, probe, one_launch_games, monkeypatch):
    one = one_launch_games
    monkeypatch.setenv("IAGO_PERSISTENT_GAMES", "0")
    loop = _play(shipped)
    assert loop["launches"] > 1
    _same(one, loop)
    assert np.array_equal(one["zn"], loop["zn"]) and np.array_equal(one["zlog"], loop["zlog"])
    ref = _play(shipped, selection="reference", z_log=False)
    assert any(not np.array_equal(ref[k], one[k]) for k in ("move", "z"))
    with selection_ref.rule():
        for g in (0, 5):
            it = iter(one["zlog"][:one["zn"][g], g])
            om = mcts_py.MCTS(probe.policy_fn, probe.value_fn, lambda s, c, it=it: int(next(it)), lmbda=0.5, c_puct=1.0,
                              n_thr=15)
            want_moves, want_z, _ = mcts_py.selfplay_game(om, N_SIMS)
            got = [int(one["move"][t, g]) if one["valid"][t, g] else -1 for t in range(len(want_moves))]
            assert got == want_moves and one["z"][g] == want_z, g
            assert next(it, None) is None, g


def test_stream_equals_the_batch_loop(shipped, one_launch_games):
    """16 games through 8 slots: the games of two batches of 8, id for id."""
    parts = [one_launch_games, _play(shipped, base=78, z_log=False)]
    s = _play(shipped, how=16, z_log=False)
    assert s["launches"] == 1 and s["valid"].shape[1] == 16
    for G in range(16):
        b, c = parts[G // 8], G % 8
        t = int(s["game_turns"][G])
        assert t <= b["n_turns"] and not b["valid"][t:, c].any(), G
        for k in ("z", "final_p1", "final_p2"):
            assert s[k][G] == b[k][c], (G, k)
        for k in ("own", "opp", "valid", "move", "pi"):
            assert np.array_equal(s[k][:t, G], b[k][:t, c]), (G, k)


def test_role_split_equals_the_single_launch(shipped, one_launch_games):
    split = _play(shipped, z_log=False, engine_kw=dict(split=8))
    single = _play(shipped, z_log=False, engine_kw=dict(split=0))
    assert split["split"] and not single["split"] and split["launches"] == single["launches"] == 1
    _same(split, single)
    _same(split, one_launch_games)


# ---- 4. the wave search
@pytest.mark.parametrize("wave", [8, 32])
def test_wave_search_bit_exact_vs_wave_mcts(shipped, golden_rules, wave):
    """Two trees (the start position and a midgame), 64 playouts, update_with_move, 60 from the other side."""
    from tests import test_search_wave_gpu as tw
    po, pp = _positions(24, golden_rules)
    own, opp = np.array([tw.START_OWN, po[13]], np.uint64), np.array([tw.START_OPP, pp[13]], np.uint64)
    active = torch.ones(2, dtype=torch.uint8, device="cuda")
    m = tw._engine(shipped, 2, 64, wave=wave, selection="alphazero")
    first, second, mv = tw._two_searches(m, own, opp, active, 64)
    assert np.all(first["zn"] == 64) and np.all(second["zn"] == 60)
    with selection_ref.rule():
        tw._oracle_check(shipped, m, own, opp, first, second, mv, [0, 1], 64, 60, wave, 1.0)
    assert int(tw._vv(m).abs().sum().item()) == 0
    assert int(m.tree.overflow.sum().item()) == 0 and int(m._ps["ctl"][3].item()) == 0
    ref = tw._engine(shipped, 2, 64, wave=wave)
    tw._two_searches(ref, own, opp, active, 64)
    assert any(m.tree.dump(g, max_depth=64) != ref.tree.dump(g, max_depth=64) for g in (0, 1))
    m.close()
    ref.close()


# ---- 5. the arena: A "alphazero", B "reference"
def _arena(shipped, one_launch, spy):
    engine, ops, policy, value, rw = shipped
    G = 8
    torch.manual_seed(4)
    from iago_amd import network
    pairs = dict(a=(policy, value), b=(network.SLPolicy().cuda().eval(), network.Value().cuda().eval()))
    ms = {}
    for who, selection in (("a", "alphazero"), ("b", "reference")):
        ms[who] = engine.BatchedMCTS(G, pairs[who][0], pairs[who][1], rw, n_thr=15, capacity=engine.suggest_capacity(N_SIMS, 15),
                                     seed=11 if who == "a" else 12, game_id_base=300 if who == "a" else 9000,
                                     persistent=True, selection=selection, z_log_rows=64 * N_SIMS)
    arena = engine.ArenaEngine(ms["a"], ms["b"])
    dumps, inner = [], arena._search_both

    def watched(sides, own, opp, one):
        n = inner(sides, own, opp, one)
        if spy and len(dumps) < 2:     # turn 0: A searched game 0; turn 1: B did
            dumps.append(ms["ab"[len(dumps)]].tree.dump(0, max_depth=64))
        return n

    arena._search_both = watched
    r = arena.play(N_SIMS, one_launch=one_launch)
    out = {k: getattr(r, k).cpu().numpy() for k in RECORDS + ("agent", "a_colour")}
    out.update(n_turns=r.n_turns, arena_launches=arena.n_arena_launches, dumps=dumps, pairs=pairs,
               zlog={w: ms[w].z_log.cpu().numpy().copy() for w in ms},
               zn={w: ms[w].z_log_n.cpu().numpy().copy() for w in ms},
               gave_up=[int(m._ps["ctl"][3].item()) for m in ms.values()],
               overflow=[int(m.tree.overflow.sum().item()) for m in ms.values()])
    for m in ms.values():
        m.close()
    return out


def test_arena_alphazero_against_reference(shipped):
    from tests.test_oracle_golden import _cmp_tree
    ops = shipped[1]
    one, seq = _arena(shipped, True, True), _arena(shipped, False, False)
    _same(one, seq, RECORDS + ("agent", "a_colour", "n_turns"))
    assert one["arena_launches"] > 0 and seq["arena_launches"] == 0
    assert one["gave_up"] == seq["gave_up"] == [0, 0] and one["overflow"] == seq["overflow"] == [0, 0]
    assert one["a_colour"][0] == 1
    own, opp = one["own"].view(np.uint64), one["opp"].view(np.uint64)
    for who, turn in (("a", 0), ("b", 1)):
        probe = NetProbe(ops, *one["pairs"][who])
        assert one["valid"][turn, 0] == 1
        it = iter(one["zlog"][who][:N_SIMS, 0])      # (the agent's first search of game 0: its first records)
        om = mcts_py.MCTS(probe.policy_fn, probe.value_fn, lambda s, c, it=it: int(next(it)), lmbda=0.5, c_puct=1.0, n_thr=15)
        s = state_of(own[turn, 0], opp[turn, 0])   # (own = the mover, as colour 1 of the state)
        if who == "a":
            with selection_ref.rule():
                want = om.get_move(s, 1, N_SIMS)
        else:
            want = om.get_move(s, 1, N_SIMS)
        assert next(it, None) is None
        _cmp_tree(one["dumps"][turn], mcts_py.dump_tree(om.root, max_depth=64), "%s g0" % who)
        if who == "a":
            _priors_exact(one["dumps"][turn], mcts_py.dump_tree(om.root, max_depth=64), "a g0")
        assert int(one["move"][turn, 0]) == want, who
    # each agent's rows are those of its own rule: two games to their end (A colour 1 in game 0, colour 2 in game 4)
    probes = {who: NetProbe(ops, *one["pairs"][who]) for who in "ab"}
    for g in (0, 4):
        searched = _replay_arena_game(one, g, probes)
        print("arena game %d: A searched %d turns, B %d" % (g, searched["a"], searched["b"]))
        assert searched["a"] >= 10 and searched["b"] >= 10


def _replay_arena_game(s, g, probes):
    """Game g of an arena to its end in the turn structure of mcts_py.selfplay_game, one oracle MCTS per agent: A's under
    selection_ref.rule(), B's outside it, each fed its own engine's z_log; BOTH advance by every move and every pass
    (update_with_move), so from its second search on an agent carries the subtree its own rule built.  Every searched
    turn: the mover's move and its visit row.  Returns the turns each agent searched."""
    from tests.forced_ref import raw_row
    ac = int(s["a_colour"][g])
    its = {w: iter(s["zlog"][w][:s["zn"][w][g], g]) for w in "ab"}
    oms = {w: mcts_py.MCTS(probes[w].policy_fn, probes[w].value_fn, lambda st, c, it=its[w]: int(next(it)), lmbda=0.5,
                           c_puct=1.0, n_thr=15) for w in "ab"}
    state = orc.initial_state()
    stone_num, pass_flg, t, searched = 4, False, 0, dict(a=0, b=0)
    while stone_num < 64:
        for color in (1, 2):
            who = "a" if color == ac else "b"
            assert int(s["agent"][t, g]) == (0 if who == "a" else 1), (g, t)
            acts = orc.legal_actions(state, color)
            if len(acts) > 0:
                assert s["valid"][t, g] == 1, (g, t)
                if who == "a":
                    with selection_ref.rule():
                        a = oms[who].get_move(state, color, N_SIMS)
                else:
                    a = oms[who].get_move(state, color, N_SIMS)
                assert int(s["move"][t, g]) == a, (g, t, who)
                assert np.array_equal(s["pi"][t, g], raw_row(oms[who].root)), (g, t, who)
                searched[who] += 1
                orc.place_stone(state, a, color)
                stone_num += 1
                pass_flg = False
            else:
                assert s["valid"][t, g] == 0 and int(s["move"][t, g]) == -1, (g, t)
                a = -1
                if pass_flg:
                    stone_num = 64
                pass_flg = True
            for om in oms.values():
                om.update_with_move(a)
            t += 1
    assert not s["valid"][t:, g].any() and s["z"][g] == orc.judge(state, 1), g
    for w in "ab":
        assert next(its[w], None) is None, (g, w)      # every recorded playout was replayed, none is missing
    return searched


# ---- 6. composition
@pytest.mark.parametrize("name,kw", [("explore", dict(explore_turns=4)), ("cap", dict(playout_cap=(5, 64), n_thr=4)),
                                     ("cap15", dict(playout_cap=(18, 64))), ("solve", dict(solve_empties=6))])
def test_composed_one_launch_equals_the_turn_loop(shipped, monkeypatch, name, kw):
    """(The cap's fast turns have 5 playouts: a root must have its children by then, so n_thr is 4 there -- the root
    expands at its fifth descent -- and 15 elsewhere; "cap15" is the cap at the default threshold, 18 fast playouts.)"""
    one = _play(shipped, z_log=False, **kw)
    assert one["replayed"] == 0 and one["launches"] == (2 if name == "solve" else 1)
    monkeypatch.setenv("IAGO_PERSISTENT_GAMES", "0")
    loop = _play(shipped, z_log=False, **kw)
    assert loop["launches"] > 2
    _same(one, loop)


def test_composed_with_root_noise_and_forced_playouts():
    """Eight roots (four at the start position, four at a midgame of 17 or more moves), one searched turn under
    root_noise (77, 128) and forced_playouts 512, random-init nets: the trees, the root children's stored priors after the
    mix to the bit -- noise_mix of the policy's own output --, and the pruned rows (BatchedMCTS.pruned_visits: the pruning
    entry point under the rule) against ForcedMCTS under the rule."""
    from tests import test_forced_gpu as tf
    from tests.gpu_util import random_positions
    from iago_amd import engine, network, ops
    torch.manual_seed(3)
    flags = []

    def make(*a, **kw):
        """An "alphazero" engine whose close() first notes whether a launch gave up and whether a pool overflowed."""
        m = engine.BatchedMCTS(*a, selection="alphazero", **kw)
        inner = m.close

        def close():
            flags.append((int(m._ps["ctl"][3].item()), int(m.tree.overflow.sum().item())))
            inner()

        m.close = close
        return m

    nets = (types.SimpleNamespace(BatchedMCTS=make,
                                  SelfPlayEngine=engine.SelfPlayEngine, suggest_capacity=engine.suggest_capacity),
            ops, network.SLPolicy().cuda().eval(), network.Value().cuda().eval())
    g = load_json("simulate.json")
    nets = nets + (ops.RolloutWeights(g["shipped_w"], g["shipped_b"]),)
    probe = NetProbe(nets[1], nets[2], nets[3])
    po, pp = random_positions(400, seed=34)
    wide = max(range(400), key=lambda i: (len(orc.legal_actions(state_of(po[i], pp[i]), 1)), -i))
    assert len(orc.legal_actions(state_of(po[wide], pp[wide]), 1)) >= 17
    own = [tf.START_OWN] * 4 + [int(po[wide])] * 4
    opp = [tf.START_OPP] * 4 + [int(pp[wide])] * 4
    with selection_ref.rule():
        forced, _, pruned = tf._run_turns(nets, probe, own, opp, 1, tf.N_SIMS, tf.NOISE, 1, False)
    print("selections a forced child won %d, rows pruned %d of 8" % (forced, pruned))
    assert forced > 0 and pruned > 0
    assert flags == [(0, 0)]


# ---- 7. refusals on the device
def test_refusals(shipped):
    engine, ops, policy, value, rw = shipped
    for kw in (dict(persistent=False), dict(use_graph=True)):
        with pytest.raises(ValueError, match="alphazero"):
            engine.BatchedMCTS(8, policy, value, rw, selection="alphazero", **kw)
    m = engine.BatchedMCTS(8, policy, value, rw, selection="alphazero", persistent=True, capacity=512)
    before = m.tree.nodes.clone()
    m.rollout_hook = lambda e: None
    own = torch.full((8,), 0x0000000810000000, dtype=torch.int64, device="cuda")
    opp = torch.full((8,), 0x0000001008000000, dtype=torch.int64, device="cuda")
    act = torch.ones(8, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="alphazero"):
        m.search(own, opp, act, N_SIMS)
    assert torch.equal(m.tree.nodes, before) and m.sim_counter == 0
    m.rollout_hook = None
    m.search(own, opp, act, N_SIMS)
    assert int(m.tree.n_visits[0].item()) == N_SIMS
    m.close()
    m = engine.BatchedMCTS(8, policy, value, rw, selection="reference", persistent=False)
    assert not m.persistent and m.selection == "reference"
    m.close()
