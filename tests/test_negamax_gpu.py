"""The negamax backup rule of the persistent search (engine.BatchedMCTS(backup="negamax"); IAGO_SEARCH_NEGAMAX in
include/iago_hip_serving.h; csrc/mcts_dev.hpp backup_value, csrc/search_kernel.hip backup_game) against its restatement
(tests/negamax_ref.py: the oracle's update_recursive starting with -leaf_value at the leaf and negating once per parent),
bit for bit, in every form that runs through backup_game: single searches with subtree reuse at n_thr 15 and 1, roots
whose paths end in pass chains (jumped over and walked), whole games in one launch / through the turn loop / as a stream,
the role split, the wave search, an arena of a negamax agent against a reference agent, and composed with exploring
openings, the playout cap, the exact endgame, root noise and forced playouts.  backup="reference" is the engine of
before, dump for dump.  Every reference is fed the search's own z_log and the production nets on one board (NetProbe)."""
import functools
import os
import types

import numpy as np
import pytest
import torch

from oracle import mcts_py
from oracle import oracle as orc
from tests import negamax_ref
from tests.conftest import GOLDEN, load_json
from tests.gpu_util import state_of
from tests.test_mcts_production_gpu import NetProbe, _positions
from tests.test_oracle_golden import _cmp_tree

pytestmark = pytest.mark.gpu

RECORDS = ("own", "opp", "valid", "move", "pi", "z", "final_p1", "final_p2")


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


def _negamax_nets(nets):
    """The nets tuple of another test module's helpers with its engine module building negamax engines."""
    engine = nets[0]
    shim = types.SimpleNamespace(BatchedMCTS=functools.partial(engine.BatchedMCTS, backup="negamax"),
                                 SelfPlayEngine=engine.SelfPlayEngine, suggest_capacity=engine.suggest_capacity)
    return (shim,) + tuple(nets[1:])


# ---- 1. trees: two searches with update_with_move between them
def _two_searches(shipped, own, opp, n_thr, n_sims=100, n_sims2=37, **kw):
    engine, ops, policy, value, rw = shipped
    G = len(own)
    m = engine.BatchedMCTS(G, policy, value, rw, lmbda=0.5, c_puct=1.0, n_thr=n_thr, seed=5, game_id_base=1000,
                           capacity=engine.suggest_capacity(n_sims + n_sims2, n_thr, moves=2), persistent=True,
                           z_log_rows=max(n_sims, n_sims2), **kw)
    assert m.persistent
    o, p = ops.bits_to_tensor(own), ops.bits_to_tensor(opp)
    active = torch.ones(G, dtype=torch.uint8, device="cuda")
    m.search(o, p, active, n_sims)
    out = dict(move=m.best_move(active)[0].cpu().numpy().copy(), z1=m.z_log.cpu().numpy().copy(),
               first=[m.tree.dump(g, max_depth=64) for g in range(G)])
    assert np.all(m.z_log_n.cpu().numpy() == n_sims)
    mv = torch.from_numpy(np.where(out["move"] == -2, -1, out["move"]).astype(np.int8)).cuda()
    m.update_with_move(mv, active.clone())
    ops.apply_moves(o, p, mv)
    m.z_log_n.zero_()
    if n_sims2:
        m.search(p, o, active, n_sims2)   # the other side is to move now
    out.update(mv=mv.cpu().numpy(), z2=m.z_log.cpu().numpy().copy(), second=[m.tree.dump(g, max_depth=64) for g in range(G)],
               skipped=int(m._ps["totals"][16].item()) if m.chain_skip else 0,
               flag=m._search_args(o, p, active, 1)[0].games_per_workgroup)
    assert int(m.tree.overflow.sum().item()) == 0 and int(m._ps["ctl"][3].item()) == 0
    m.close()
    return out


def _reference_check(probe, got, own, opp, games, n_thr, n_sims=100, n_sims2=37):
    """The games' trees after both searches against oracle.mcts_py.MCTS under whatever rule Node.update_recursive is."""
    for g in games:
        it = iter(got["z1"][:n_sims, g])
        om = mcts_py.MCTS(probe.policy_fn, probe.value_fn, lambda s, c, it=it: int(next(it)), lmbda=0.5, c_puct=1.0,
                          n_thr=n_thr)
        s = state_of(own[g], opp[g])
        want = om.get_move(s, 1, n_sims)
        assert next(it, None) is None
        _cmp_tree(got["first"][g], mcts_py.dump_tree(om.root, max_depth=64), "g%d" % g)
        assert got["move"][g] == (-2 if want is None else want), g
        if not n_sims2:
            continue
        a = int(got["mv"][g])
        om.update_with_move(a)
        orc.place_stone(s, a, 1)
        it = iter(got["z2"][:n_sims2, g])
        om.rollout_fn = lambda st, c, it=it: int(next(it))
        om.get_move(s, 2, n_sims2)
        assert next(it, None) is None
        _cmp_tree(got["second"][g], mcts_py.dump_tree(om.root, max_depth=64), "g%d'" % g)


@pytest.mark.parametrize("n_thr", [15, 1])
def test_trees_bit_exact_vs_the_negamax_reference(shipped, probe, golden_rules, n_thr):
    """24 games -- start positions, midgames, 'pass1' / 'dead' / 'full' at 1 / 2 / 3 --, 100 playouts, update_with_move,
    37 more from the other side.  n_thr 1: a node expands at its first visit, so the paths are deep and end at both
    parities many times over.  Ten games against the reference; backup="reference" is the engine without the argument."""
    from iago_amd import _lib
    own, opp = _positions(24, golden_rules)
    neg = _two_searches(shipped, own, opp, n_thr, backup="negamax")
    ref = _two_searches(shipped, own, opp, n_thr, backup="reference")
    old = _two_searches(shipped, own, opp, n_thr)
    assert neg["flag"] & _lib.SEARCH_NEGAMAX and not (ref["flag"] | old["flag"]) & _lib.SEARCH_NEGAMAX
    for k in ("first", "second"):
        assert ref[k] == old[k], k                        # dump for dump, every game
    assert np.array_equal(ref["move"], old["move"]) and np.array_equal(ref["z1"], old["z1"])
    checked = [0, 1, 2, 3, 4, 12, 13, 14, 15, 16]
    with negamax_ref.rule():
        _reference_check(probe, neg, own, opp, checked, n_thr)
    differ = [g for g in checked if neg["second"][g] != ref["second"][g]]
    print("n_thr %d: %d of %d checked trees differ from the reference rule's" % (n_thr, len(differ), len(checked)))
    assert differ


# ---- 2. pass chains
def test_pass_chains_jumped_and_walked(shipped, probe):
    """Roots with 0 .. 3 empties (the mover has a move, must pass, or the game is over): the paths end in chains of pass
    levels, which the descent jumps over by path index -- the parity is the walk's."""
    from tests.test_pass_chain_skip_gpu import _late_roots, _roots
    found = _late_roots()
    assert sum(1 for k in found if 1 <= k[0] <= 3) >= 4, sorted(found)
    own, opp = _roots(found, 8)
    on = _two_searches(shipped, own, opp, 15, n_sims2=0, backup="negamax", chain_skip=True)
    off = _two_searches(shipped, own, opp, 15, n_sims2=0, backup="negamax", chain_skip=False)
    assert on["skipped"] > 0 and off["skipped"] == 0
    assert on["first"] == off["first"] and np.array_equal(on["z1"], off["z1"])
    with negamax_ref.rule():
        _reference_check(probe, on, own, opp, range(8), 15, n_sims2=0)
    ref = _two_searches(shipped, own, opp, 15, n_sims2=0)
    assert any(on["first"][g] != ref["first"][g] for g in range(8))


# ---- 3. / 4. / 7. whole games
def _play(shipped, G=8, n_sims=24, how="play", base=70, z_log=True, n_thr=15, engine_kw=None, **kw):
    engine, ops, policy, value, rw = shipped
    m = engine.BatchedMCTS(G, policy, value, rw, n_thr=n_thr, capacity=4096, seed=11, game_id_base=base, persistent=True,
                           backup="negamax", **(dict(z_log_rows=128 * n_sims) if z_log else {}), **(engine_kw or {}))
    e = engine.SelfPlayEngine(m)
    r = e.play(n_sims, **kw) if how == "play" else e.play_stream(n_sims, how, **kw)
    out = {k: getattr(r, k).cpu().numpy() for k in RECORDS}
    out["game_turns"] = r.game_turns.cpu().numpy() if r.game_turns is not None else None
    out.update(n_turns=r.n_turns, launches=r.launches, replayed=e.n_replayed, split=m._split is not None,
               gave_up=int(m._ps["ctl"][3].item()))
    if z_log:
        out["zlog"], out["zn"] = m.z_log.cpu().numpy().copy(), m.z_log_n.cpu().numpy().copy()
    m.close()
    return out


def _same(a, b, keys=RECORDS + ("n_turns",)):
    for k in keys:
        assert np.array_equal(a[k], b[k]), k


@pytest.fixture(scope="module")
def one_launch_games(shipped):
    out = _play(shipped)
    assert out["launches"] == 1 and out["replayed"] == 0
    return out


def test_whole_games_one_launch_turn_loop_and_reference(shipped, probe, one_launch_games, monkeypatch):
    one = one_launch_games
    monkeypatch.setenv("IAGO_PERSISTENT_GAMES", "0")
    loop = _play(shipped)
    assert loop["launches"] > 1
    _same(one, loop)
    assert np.array_equal(one["zn"], loop["zn"]) and np.array_equal(one["zlog"], loop["zlog"])
    with negamax_ref.rule():
        for g in range(8):
            it = iter(one["zlog"][:one["zn"][g], g])
            om = mcts_py.MCTS(probe.policy_fn, probe.value_fn, lambda s, c, it=it: int(next(it)), lmbda=0.5, c_puct=1.0,
                              n_thr=15)
            want_moves, want_z, _ = mcts_py.selfplay_game(om, 24)
            got = [int(one["move"][t, g]) if one["valid"][t, g] else -1 for t in range(len(want_moves))]
            assert got == want_moves and one["z"][g] == want_z, g
            assert next(it, None) is None, g


def test_stream_equals_the_batch_loop(shipped, one_launch_games):
    parts = [one_launch_games] + [_play(shipped, base=70 + 8 * k, z_log=False) for k in (1, 2)]
    s = _play(shipped, how=24, z_log=False)
    assert s["launches"] == 1 and s["gave_up"] == 0 and s["valid"].shape[1] == 24
    for G in range(24):
        b, c = parts[G // 8], G % 8
        t = int(s["game_turns"][G])
        assert t <= b["n_turns"] and not b["valid"][t:, c].any(), G
        for k in ("z", "final_p1", "final_p2"):
            assert s[k][G] == b[k][c], (G, k)
        for k in ("own", "opp", "valid", "move", "pi"):
            assert np.array_equal(s[k][:t, G], b[k][:t, c]), (G, k)


def test_a_replayed_batch_equals_the_turn_loop(shipped, monkeypatch):
    """A pool that passes play()'s test (made lenient here, as tests/test_search_persistent_gpu.py does) but cannot hold
    what the games leave behind: the launch reports the full pool and the batch is replayed turn by turn -- under the
    same rule, so the games are those of a pool that holds them.  Random-init nets: broad trees."""
    from iago_amd import network
    engine, ops, _, _, rw = shipped
    torch.manual_seed(3)
    policy, value = network.SLPolicy().cuda().eval(), network.Value().cuda().eval()
    G, n_sims = 16, 60

    def play(cap, backup="negamax"):
        m = engine.BatchedMCTS(G, policy, value, rw, n_thr=15, capacity=cap, seed=9, persistent=True, backup=backup)
        e = engine.SelfPlayEngine(m)
        r = e.play(n_sims)
        out = {k: getattr(r, k).cpu().numpy() for k in RECORDS}
        out.update(n_turns=r.n_turns, replayed=e.n_replayed, one_launch=r.game_turns is not None,
                   used=int(m.tree.n_nodes.max().item()), compactions=m.n_compactions)
        m.close()
        return out

    big = play(engine.suggest_capacity(n_sims, 15))
    assert big["replayed"] == 0 and big["one_launch"] and big["used"] > 256
    monkeypatch.setattr(engine, "suggest_capacity", lambda *a, **k: 64)
    small = play(256)
    assert small["replayed"] == 1 and not small["one_launch"] and small["compactions"] > 0
    _same(small, big)
    ref = play(256, backup="reference")
    assert any(not np.array_equal(ref[k], small[k]) for k in ("move", "z"))   # (the replay kept the rule)


def test_role_split_equals_the_single_launch(shipped):
    """96 games on 8 game CUs (two game workgroups per CU) against the single launch."""
    split = _play(shipped, G=96, z_log=False, engine_kw=dict(split=8))
    single = _play(shipped, G=96, z_log=False, engine_kw=dict(split=0))
    assert split["split"] and not single["split"] and split["gave_up"] == single["gave_up"] == 0
    assert split["launches"] == single["launches"] == 1
    _same(split, single)


@pytest.mark.parametrize("name,kw", [("explore", dict(explore_turns=8)), ("cap", dict(playout_cap=(18, 64))),
                                     ("solve", dict(solve_empties=8))])
def test_composed_one_launch_equals_the_turn_loop(shipped, monkeypatch, name, kw):
    one = _play(shipped, z_log=False, **kw)
    assert one["replayed"] == 0 and one["launches"] == (2 if name == "solve" else 1)
    monkeypatch.setenv("IAGO_PERSISTENT_GAMES", "0")
    loop = _play(shipped, z_log=False, **kw)
    assert loop["launches"] > 2
    _same(one, loop)


def test_composed_with_root_noise_and_forced_playouts(shipped, probe):
    """Four games, two consecutive searched turns: trees and pruned rows against ForcedMCTS under the negamax rule."""
    from tests import test_forced_gpu as tf
    own, opp = [tf.START_OWN] * 4, [tf.START_OPP] * 4
    with negamax_ref.rule():
        forced, reused, pruned = tf._run_turns(_negamax_nets(shipped), probe, own, opp, 1, tf.N_SIMS, tf.NOISE, 2, False)
    assert forced > 0 and reused >= 4 and pruned > 0


# ---- 5. the wave search
@pytest.mark.parametrize("wave", [8, 32])
def test_wave_search_bit_exact_vs_wave_mcts(shipped, wave):
    from tests import test_search_wave_gpu as tw
    own, opp = np.array([tw.START_OWN], np.uint64), np.array([tw.START_OPP], np.uint64)
    active = torch.ones(1, dtype=torch.uint8, device="cuda")
    m = tw._engine(shipped, 1, 128, wave=wave, backup="negamax")
    first, second, mv = tw._two_searches(m, own, opp, active, 128)
    with negamax_ref.rule():
        tw._oracle_check(shipped, m, own, opp, first, second, mv, [0], 128, 60, wave, 1.0)
    assert int(tw._vv(m).abs().sum().item()) == 0
    ref = tw._engine(shipped, 1, 128, wave=wave)
    tw._two_searches(ref, own, opp, active, 128)
    assert m.tree.dump(0, max_depth=64) != ref.tree.dump(0, max_depth=64)
    m.close()
    ref.close()


# ---- 6. the arena: A negamax, B the reference's rule
def _arena(shipped, one_launch, spy):
    engine, ops, policy, value, rw = shipped
    G, n_sims = 16, 24
    torch.manual_seed(4)
    from iago_amd import network
    pairs = dict(a=(policy, value), b=(network.SLPolicy().cuda().eval(), network.Value().cuda().eval()))
    ms = {}
    for who, backup in (("a", "negamax"), ("b", "reference")):
        ms[who] = engine.BatchedMCTS(G, pairs[who][0], pairs[who][1], rw, n_thr=15, capacity=engine.suggest_capacity(n_sims, 15),
                                     seed=11 if who == "a" else 12, game_id_base=300 if who == "a" else 9000,
                                     persistent=True, backup=backup, z_log_rows=64 * n_sims)
    arena = engine.ArenaEngine(ms["a"], ms["b"])
    dumps, inner = [], arena._search_both

    def watched(sides, own, opp, one):
        n = inner(sides, own, opp, one)
        if spy and len(dumps) < 2:     # turn 0: A searched games 0 and 1; turn 1: B did
            who = "ab"[len(dumps)]
            dumps.append([ms[who].tree.dump(g, max_depth=64) for g in (0, 1)])
        return n

    arena._search_both = watched
    r = arena.play(n_sims, one_launch=one_launch)
    out = {k: getattr(r, k).cpu().numpy() for k in RECORDS + ("agent", "a_colour")}
    out.update(n_turns=r.n_turns, arena_launches=arena.n_arena_launches, dumps=dumps, pairs=pairs,
               zlog={w: ms[w].z_log.cpu().numpy().copy() for w in ms},
               gave_up=[int(m._ps["ctl"][3].item()) for m in ms.values()])
    for m in ms.values():
        m.close()
    return out


def test_arena_negamax_against_reference(shipped):
    ops = shipped[1]
    one, seq = _arena(shipped, True, True), _arena(shipped, False, False)
    _same(one, seq, RECORDS + ("agent", "a_colour", "n_turns"))
    assert one["arena_launches"] > 20 and seq["arena_launches"] == 0 and one["gave_up"] == seq["gave_up"] == [0, 0]
    assert np.all(one["a_colour"][:2] == 1)
    own, opp = one["own"].view(np.uint64), one["opp"].view(np.uint64)
    for who, turn, colour in (("a", 0, 1), ("b", 1, 2)):
        probe = NetProbe(ops, *one["pairs"][who])
        for g in (0, 1):
            assert one["valid"][turn, g] == 1
            it = iter(one["zlog"][who][:24, g])      # (the agent's first search of the game: its first 24 records)
            om = mcts_py.MCTS(probe.policy_fn, probe.value_fn, lambda s, c, it=it: int(next(it)), lmbda=0.5, c_puct=1.0,
                              n_thr=15)
            s = state_of(own[turn, g], opp[turn, g])   # (own = the mover, as colour 1 of the state)
            if who == "a":
                with negamax_ref.rule():
                    want = om.get_move(s, 1, 24)
            else:
                want = om.get_move(s, 1, 24)
            assert next(it, None) is None
            _cmp_tree(one["dumps"][turn][g], mcts_py.dump_tree(om.root, max_depth=64), "%s g%d" % (who, g))
            assert int(one["move"][turn, g]) == want, (who, g)


# ---- 8. refusals
def test_refusals(shipped):
    engine, ops, policy, value, rw = shipped
    for kw in (dict(persistent=False), dict(use_graph=True)):
        with pytest.raises(ValueError, match="negamax"):
            engine.BatchedMCTS(8, policy, value, rw, backup="negamax", **kw)
    with pytest.raises(ValueError, match="backup"):
        engine.BatchedMCTS(8, policy, value, rw, backup="minimax")
    # a rollout hook, set after construction, would send the searches through the per-playout launches: refused where a
    # search or a round of games begins, the trees untouched
    m = engine.BatchedMCTS(8, policy, value, rw, backup="negamax", persistent=True, capacity=512)
    before = m.tree.nodes.clone()
    m.rollout_hook = lambda e: None
    own = torch.full((8,), 0x0000000810000000, dtype=torch.int64, device="cuda")
    opp = torch.full((8,), 0x0000001008000000, dtype=torch.int64, device="cuda")
    act = torch.ones(8, dtype=torch.uint8, device="cuda")
    e = engine.SelfPlayEngine(m)
    for call in (lambda: m.search(own, opp, act, 20), lambda: e.play(20), lambda: e.play_stream(20, 16),
                 lambda: e.play_match(20)):
        with pytest.raises(ValueError, match="negamax"):
            call()
    assert torch.equal(m.tree.nodes, before) and m.sim_counter == 0
    m.rollout_hook = None
    m.search(own, opp, act, 20)
    assert int(m.tree.n_visits[0].item()) == 20
    m.close()
    # (a per-playout engine with the reference's rule is today's)
    m = engine.BatchedMCTS(8, policy, value, rw, backup="reference", persistent=False)
    assert not m.persistent and m.backup == "reference"
    m.close()
