"""The Gumbel root search on the GPU (BatchedMCTS.search(gumbel=) / gumbel_move / gumbel_rows, SelfPlayEngine.play /
play_match(gumbel=), engine.gumbel_targets; iago_mcts_gumbel_draw, iago_mcts_search_gumbel, iago_mcts_gumbel_finish)
against tests/gumbel_ref.py, bit for bit: the draw kernel alone; the trees, moves and rows of two consecutive searched
turns against the oracle subclass fed the recorded z; roots with one move or none; a root that was not fresh (the rule's
fallback); whole games through the turn loop replayed game by game, alone and with the endgame solver, the playout cap and
an alpha-beta opponent; the role split against the single launch.  Sizes after tests/test_negamax_gpu.py's: 8 slots, the shipped nets, n_thr 1, capacity 4096."""
import os

import numpy as np
import pytest
import torch

from oracle import mcts_py
from oracle import oracle as orc
from tests import gumbel_ref as gr, negamax_ref, playout_cap_ref as cap_ref, selection_ref
from tests.conftest import GOLDEN, load_json
from tests.gpu_util import random_positions, state_of
from tests.test_mcts_production_gpu import NetProbe
from tests.test_oracle_golden import _cmp_tree

pytestmark = pytest.mark.gpu

SLOTS, BASE, S0, SEED = 8, 300, 1000, 11
GUMBEL = (4, 256)
CAP = (8, 64)
START_OWN, START_OPP = 0x0000000810000000, 0x0000001008000000
RECORDS = ("own", "opp", "valid", "move", "pi", "pi_raw", "z", "final_p1", "final_p2")


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


@pytest.fixture(scope="module")
def tables(shipped):
    return shipped[1].gumbel_tables()


@pytest.fixture(scope="module")
def wide():
    """A reachable position of an oracle game with 9 or more legal moves: more than m = 8."""
    own, opp = random_positions(200, seed=34)
    for o, p in zip(own, opp):
        if len(orc.legal_actions(state_of(o, p), 1)) >= 9:
            return int(o), int(p)
    raise AssertionError("no wide position")


def _engine(shipped, slots=SLOTS, base=BASE, **kw):
    engine, ops, policy, value, rw = shipped
    kw.setdefault("backup", "negamax")
    kw.setdefault("selection", "alphazero")
    m = engine.BatchedMCTS(slots, policy, value, rw, n_thr=1, seed=SEED, game_id_base=base, persistent=True, capacity=4096,
                           **kw)
    m.sim_counter = S0
    return m


def _oracle(probe, tables, game_id, gumbel=GUMBEL):
    return gr.GumbelMCTS(probe.policy_fn, probe.value_fn, None, lmbda=0.5, c_puct=1.0, n_thr=1,
                         gumbel=tuple(gumbel) + (gr.C_VISIT,), tables=tables, seed=SEED, game_id=game_id)


def _same_rows(got, om, where):
    """The device's three rows (n, q, logit) of one game against the oracle subclass's, the float32 q to the bit."""
    n, q, lg = om.rows()
    assert np.array_equal(got[0], n), where
    assert got[1].astype(np.float32).tobytes() == q.tobytes(), where
    assert np.array_equal(got[2], lg), where


def _same_root_priors(dump, om, where):
    got = [np.float32(dump["children"][str(a)]["P"]).tobytes() for a in dump["order"]]
    assert got == [np.float32(ch.P).tobytes() for ch in om.root.children.values()], where


# ---- 1. the draw kernel alone
def test_the_draw_kernel_equals_the_numpy_draw(shipped, tables):
    m = _engine(shipped)
    st = m._gumbel_state()
    for turn in (0, 5):
        ids, turns = m._turn_ids(turn)
        st["g"].fill_(0x7777777)
        active = torch.ones(SLOTS, dtype=torch.uint8, device="cuda")
        active[6] = 0
        shipped[1].gumbel_draw(m.tree.ref(), active, SEED, ids, turns, (16, 256, 50), st["tables"], st["g"])
        got = st["g"].cpu().numpy()
        for g in range(SLOTS):
            if g == 6:
                assert np.all(got[g] == 0x7777777)                       # inactive: not touched
            else:
                assert np.array_equal(got[g], gr.draw(SEED, BASE + g, turn, tables[0])), (g, turn)
    assert np.array_equal(st["tables"][0].cpu().numpy(), tables[0]) and np.array_equal(st["tables"][1].cpu().numpy(), tables[1])
    m.close()


# ---- 2. two searched turns: trees, moves and rows against the oracle subclass, z replayed
@pytest.mark.parametrize("n_sims,m_", [(16, 4), (37, 16), (5, 8)])
def test_two_searched_turns_bit_exact_vs_the_oracle_subclass(shipped, probe, tables, wide, n_sims, m_):
    """Four games from the start position (4 legal moves: fewer than m = 16 and 8) and four from a position with 9 or more
    (more than m = 8 and 4).  (5, 8): a budget smaller than m."""
    engine, ops = shipped[0], shipped[1]
    own, opp = [START_OWN] * 4 + [wide[0]] * 4, [START_OPP] * 4 + [wide[1]] * 4
    G = len(own)
    m = _engine(shipped, z_log_rows=n_sims)
    oms = [_oracle(probe, tables, BASE + g, (m_, 256)) for g in range(G)]
    states, colors = [state_of(own[g], opp[g]) for g in range(G)], [1] * G
    o, p = ops.bits_to_tensor(own), ops.bits_to_tensor(opp)
    m.tree.reset()
    ks = set()
    with negamax_ref.rule(), selection_ref.rule():
        for t in range(2):
            acts = [orc.legal_actions(states[g], colors[g]) for g in range(G)]
            active = torch.tensor([1 if a else 0 for a in acts], dtype=torch.uint8, device="cuda")
            m.z_log_n.zero_()
            m.search(o, p, active, n_sims, gumbel=(m_, 256), turn=t)
            zlog = m.z_log.cpu().numpy()
            rows = [x.cpu().numpy().copy() for x in m.gumbel_rows(active)]
            move = m.move.cpu().numpy().copy()
            assert np.array_equal(move, m.gumbel_move(active).cpu().numpy())
            raw = m.best_move(active)[1].cpu().numpy().copy()
            for g in range(G):
                om = oms[g]
                if not acts[g]:
                    move[g] = -1
                    om.update_with_move(-1)
                    continue
                it = iter(zlog[:n_sims, g])
                om.rollout_fn = lambda s, c, it=it: int(next(it))
                om.begin_turn(t)
                want = om.get_move(states[g], colors[g], n_sims)
                assert next(it, None) is None and om.fallbacks == 0
                d = m.tree.dump(g, max_depth=64)
                _cmp_tree(d, mcts_py.dump_tree(om.root, max_depth=64), "g%d t%d" % (g, t))
                _same_root_priors(d, om, (g, t))
                assert move[g] == want, (g, t, move[g], want)
                _same_rows([r[g] for r in rows], om, (g, t))
                assert np.array_equal(raw[g], om.raw_row()), (g, t)
                ks.add(len(acts[g]))
                om.update_with_move(int(want))
                orc.place_stone(states[g], int(want), colors[g])
            mv = torch.from_numpy(move.astype(np.int8)).cuda()
            m.update_with_move(mv, torch.ones(G, dtype=torch.uint8, device="cuda"))
            ops.apply_moves(o, p, mv)
            o, p = p, o
            colors = [3 - c for c in colors]
    assert min(ks) < m_ or m_ == 4
    assert max(ks) > m_ or m_ == 16
    m.close()


# ---- 3. one legal move, a pass, and a root that was not fresh
def test_one_move_a_pass_and_the_fallback(shipped, probe, tables, golden_rules):
    engine, ops = shipped[0], shipped[1]
    pool = random_positions(400, seed=34)
    single = next((int(o), int(q)) for o, q in zip(*pool) if len(orc.legal_actions(state_of(o, q), 1)) == 1)
    eb = golden_rules["edge_boards"]
    own = [single[0], eb[6][0]] + [START_OWN] * 6            # 'pass1': the mover must pass
    opp = [single[1], eb[6][1]] + [START_OPP] * 6
    m = _engine(shipped, z_log_rows=16)
    o, p = ops.bits_to_tensor(own), ops.bits_to_tensor(opp)
    active = torch.ones(SLOTS, dtype=torch.uint8, device="cuda")
    m.tree.reset()
    m.search(o, p, active, 16, gumbel=GUMBEL, turn=3)
    rows = [x.cpu().numpy().copy() for x in m.gumbel_rows(active)]
    move = m.move.cpu().numpy().copy()
    only = orc.legal_actions(state_of(*single), 1)[0]
    assert move[0] == only and move[1] == -1
    assert rows[0][0][only] == 15 and rows[0][0].sum() == 15 and (rows[2][0] != gr.INT32_MIN).sum() == 1
    assert rows[2][0][only] == 8                              # the lone child's p == 1.0: ln_q16[0]
    assert not rows[0][1].any() and not rows[1][1].any() and np.all(rows[2][1] == gr.INT32_MIN)
    zlog = m.z_log.cpu().numpy()
    with negamax_ref.rule(), selection_ref.rule():
        for g in (0, 1, 2):
            om = _oracle(probe, tables, BASE + g)
            it = iter(zlog[:16, g])
            om.rollout_fn = lambda s, c, it=it: int(next(it))
            om.begin_turn(3)
            assert om.get_move(state_of(own[g], opp[g]), 1, 16) == move[g], g
            _cmp_tree(m.tree.dump(g, max_depth=64), mcts_py.dump_tree(om.root, max_depth=64), "g%d" % g)
            _same_rows([r[g] for r in rows], om, g)
    # a root that was not fresh (the engine's reset bypassed): no child has the schedule's count, and the children of the
    # largest visit count are scored -- as the reference does
    m.tree.reset()
    m.z_log_n.zero_()
    m.search(o, p, active, 9)
    z1 = m.z_log.cpu().numpy().copy()
    m.z_log_n.zero_()
    m._search_persistent(o, p, active, 16, SLOTS, engine.RootRule(None, None, GUMBEL + (gr.C_VISIT,)), 1)
    z2 = m.z_log.cpu().numpy().copy()
    move = m.gumbel_move(active).cpu().numpy().copy()
    fallbacks = 0
    with negamax_ref.rule(), selection_ref.rule():
        for g in (2, 3):
            om = _oracle(probe, tables, BASE + g)
            it = iter(z1[:9, g])
            om.rollout_fn = lambda s, c, it=it: int(next(it))
            om.begin_turn(0, on=False)
            om.get_move(state_of(own[g], opp[g]), 1, 9)
            it = iter(z2[:16, g])
            om.rollout_fn = lambda s, c, it=it: int(next(it))
            om.on, om.g = True, gr.draw(SEED, BASE + g, 1, tables[0])     # (begin_turn without the fresh root)
            assert om.get_move(state_of(own[g], opp[g]), 1, 16) == move[g], g
            _cmp_tree(m.tree.dump(g, max_depth=64), mcts_py.dump_tree(om.root, max_depth=64), "g%d'" % g)
            fallbacks += om.fallbacks
    assert fallbacks > 0
    m.close()


# ---- 4. whole games through the turn loop
GAMES = {"plain": dict(), "solve": dict(solve_empties=6), "cap": dict(playout_cap=CAP)}


@pytest.fixture(scope="module")
def games(shipped):
    out = {}
    for name, kw in GAMES.items():
        m = _engine(shipped, z_log_rows=128 * 16)
        res = shipped[0].SelfPlayEngine(m).play(16, gumbel=GUMBEL, **kw)
        s = {k: getattr(res, k).cpu().numpy() for k in RECORDS}
        s.update(n_turns=res.n_turns, launches=res.launches, base=res.game_id_base, res=res,
                 zlog=m.z_log.cpu().numpy(), zn=m.z_log_n.cpu().numpy())
        m.close()
        out[name] = s
    return out


def _same_target(got, om, where):
    """A recorded pi row against the float64 reference: within 1 count, exact where no cell sits at a rounding boundary."""
    want, clear = gr.targets(*om.rows(), c_visit=gr.C_VISIT, c_scale_256=GUMBEL[1])
    assert np.abs(got.astype(np.int64) - want[0]).max() <= 1, where
    assert not clear[0] or np.array_equal(got, want[0]), where
    return bool(clear[0])


def _replay(probe, tables, s, g, capped=False, solved_from=None, mine=None):
    """Game g of a batch replayed by the oracle subclass from the searches' z record: move, pi, pi_raw and valid of every
    searched turn.  Under the cap a fast turn is the plain search's: n_fast playouts on the tree as it stands, the most
    visited child, pi = pi_raw.  mine: the colour PV-MCTS plays in a match (the other turns are played as recorded)."""
    it = iter(s["zlog"][:s["zn"][g], g])
    om = _oracle(probe, tables, s["base"] + g)
    om.rollout_fn = lambda st, c: int(next(it))
    state = orc.initial_state()
    stone_num, pass_flg, t, kinds, clear = 4, False, 0, set(), []
    while stone_num < 64:
        for color in (1, 2):
            acts = orc.legal_actions(state, color)
            if len(acts) > 0:
                v = int(s["valid"][t, g])
                if v in (2, 3, 5):
                    assert v != 3 or (solved_from is not None and int((np.asarray(state) == 0).sum()) <= solved_from), (g, t)
                    assert v == 3 or mine is not None, (g, t)
                    assert not s["pi"][t, g].any() and not s["pi_raw"][t, g].any(), (g, t)
                    a = int(s["move"][t, g])
                    assert a in acts, (g, t)
                    kinds.add({2: "drawn", 3: "solved", 5: "opening"}[v])
                else:
                    assert mine is None or color == mine, (g, t)
                    full = not capped or cap_ref.is_full(SEED, s["base"] + g, t, CAP[1])
                    om.begin_turn(t, on=full)
                    a = om.get_move(state, color, 16 if full else CAP[0])
                    assert v == (1 if full else 4), (g, t)
                    assert np.array_equal(s["pi_raw"][t, g], om.raw_row()), (g, t)
                    if full:
                        clear.append(_same_target(s["pi"][t, g], om, (g, t)))
                    else:
                        assert np.array_equal(s["pi"][t, g], s["pi_raw"][t, g]), (g, t)
                    assert s["move"][t, g] == a, (g, t)
                    kinds.add(full)
                om.update_with_move(a)
                orc.place_stone(state, a, color)
                stone_num += 1
                pass_flg = False
            else:
                assert s["valid"][t, g] == 0 and s["move"][t, g] == -1 and not s["pi_raw"][t, g].any(), (g, t)
                if pass_flg:
                    stone_num = 64
                pass_flg = True
                om.update_with_move(-1)
            t += 1
    assert next(it, None) is None, g             # the oracle consumed exactly the playouts the launches ran
    assert s["z"][g] == orc.judge(state, 1), g
    return kinds, clear


@pytest.mark.parametrize("g", range(SLOTS))
def test_whole_games_replayed_by_the_oracle_subclass(probe, tables, games, g):
    s = games["plain"]
    assert s["launches"] == s["n_turns"] > 1     # (the turn loop)
    with negamax_ref.rule(), selection_ref.rule():
        kinds, clear = _replay(probe, tables, s, g)
    assert kinds == {True} and np.mean(clear) >= 0.9


def test_role_split_plays_the_same_games(shipped, games):
    """The role split's game launch (search_game_gumbel_kernel on the CU-masked streams, the nets in a launch of their own)
    against the single launch: the same games, record for record."""
    m = _engine(shipped, split=8)
    if m._split is None:
        m.close()
        pytest.skip("this runtime gives no CU-masked streams")
    res = shipped[0].SelfPlayEngine(m).play(16, gumbel=GUMBEL)
    gave_up = int(m._ps["ctl"][3].item())
    m.close()
    s = games["plain"]
    assert gave_up == 0 and res.launches == s["launches"] and res.n_turns == s["n_turns"]
    for k in RECORDS:
        assert np.array_equal(getattr(res, k).cpu().numpy(), s[k]), k


def test_the_records_of_such_games(games):
    s = games["plain"]
    searched = s["valid"] == 1
    assert s["pi"].dtype == s["pi_raw"].dtype == np.int32 and s["pi"].shape == s["pi_raw"].shape
    assert np.all(s["pi_raw"][searched].sum(axis=1) == 15)                  # n_thr 1: the first playout expands nothing
    k = (s["pi"][searched] > 0).sum(axis=1)
    assert np.all(np.abs(s["pi"][searched].sum(axis=1) - 65536) <= 64)
    assert not s["pi"][~searched].any() and not s["pi_raw"][~searched].any() and k.max() > 1
    # the move is among the most visited
    rows, mv = s["pi_raw"][searched], s["move"][searched]
    assert np.all(rows[np.arange(len(mv)), mv] == rows.max(axis=1))


def test_composed_with_the_endgame_solver(probe, tables, games):
    s = games["solve"]
    assert (s["valid"] == 3).any()
    kinds = set()
    with negamax_ref.rule(), selection_ref.rule():
        for g in range(SLOTS):
            kinds |= _replay(probe, tables, s, g, solved_from=6)[0]
    assert kinds == {True, "solved"}


def test_under_a_playout_cap_only_the_full_turns_run_the_rule(probe, tables, games):
    s = games["cap"]
    fast = s["valid"] == 4
    assert fast.any() and (s["valid"] == 1).any()
    assert np.array_equal(s["pi"][fast], s["pi_raw"][fast])
    kinds = set()
    with negamax_ref.rule(), selection_ref.rule():
        for g in range(SLOTS):
            kinds |= _replay(probe, tables, s, g, capped=True)[0]
    assert kinds == {True, False}


def test_a_match_against_alphabeta(shipped, probe, tables):
    engine = shipped[0]
    m = _engine(shipped, z_log_rows=64 * 16)
    res = engine.SelfPlayEngine(m).play_match(16, opponent=engine.AlphaBeta(1), gumbel=GUMBEL)
    s = {k: getattr(res, k).cpu().numpy() for k in RECORDS}
    s.update(base=res.game_id_base, zlog=m.z_log.cpu().numpy(), zn=m.z_log_n.cpu().numpy())
    col = res.mcts_colour.cpu().numpy()
    m.close()
    # without records the target is not made; the games are the same
    m = _engine(shipped)
    bare = engine.SelfPlayEngine(m).play_match(16, opponent=engine.AlphaBeta(1), gumbel=GUMBEL, record=False)
    m.close()
    for k in ("z", "final_p1", "final_p2"):
        assert np.array_equal(getattr(bare, k).cpu().numpy(), s[k]), k
    assert bare.n_turns == res.n_turns
    assert res.launches == res.n_turns and np.all(col == 2)
    with negamax_ref.rule(), selection_ref.rule():
        for g in range(SLOTS):
            kinds, _ = _replay(probe, tables, s, g, mine=2)
            assert True in kinds and "drawn" in kinds, g


# ---- 5. gumbel=None is the parent's call
def test_none_is_the_play_of_before(shipped, monkeypatch):
    engine, ops = shipped[0], shipped[1]

    def host(r):
        return {k: getattr(r, k).cpu().numpy() for k in RECORDS if k != "pi_raw"}

    def play(**kw):
        m = _engine(shipped)
        r = engine.SelfPlayEngine(m).play(16, **kw)
        dumps = [m.tree.dump(g, max_depth=64) for g in range(SLOTS)]
        m.close()
        return r, dumps
    want_res, want_dumps = play()

    def never(*a, **k):
        raise AssertionError("gumbel = None reached the Gumbel root search's entry points")
    for name in ("gumbel_draw", "search_gumbel", "gumbel_finish"):
        monkeypatch.setattr(ops, name, never)
    res, dumps = play(gumbel=None)
    got, want = host(res), host(want_res)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert dumps == want_dumps and res.launches == want_res.launches and res.pi_raw is None


# ---- 6. the target kernel-free: engine.gumbel_targets on the device against the float64 reference
def test_gumbel_targets_against_the_float64_reference(shipped, games):
    engine = shipped[0]
    from tests.test_gumbel_ref_cpu import _random_rows
    n, q, lg = _random_rows(np.random.default_rng(3), 400, shipped[1].gumbel_tables())
    rows = (torch.from_numpy(n.astype(np.int32)).cuda(), torch.from_numpy(q).cuda(), torch.from_numpy(lg.astype(np.int32)).cuda())
    for c_visit, c_scale in ((50, 256), (4096, 64)):
        got = engine.gumbel_targets(rows, c_visit, c_scale)
        assert got.is_cuda and got.dtype == torch.int32
        got = got.cpu().numpy()
        want, clear = gr.targets(n, q, lg, c_visit, c_scale)
        print("share of clear rows %.4f" % clear.mean())
        assert clear.mean() >= 0.9
        assert np.abs(got.astype(np.int64) - want).max() <= 1
        assert np.array_equal(got[clear], want[clear])
        assert not got[lg == gr.INT32_MIN].any()


# ---- 7. training on the improved policy
def test_the_trainer_steps_on_the_improved_policy(shipped, games):
    from iago_amd import network
    from iago_amd.train_rl import ReinforceTrainer
    s = games["plain"]
    model = network.SLPolicy()
    model.load_state_dict(shipped[2].state_dict())
    tr = ReinforceTrainer(model, pool_dir=None, N=2, seed=1)
    out = tr.step_from_tuples(s["res"].tuples(), target="visits")
    assert out["n_tuples"] == int((s["valid"] == 1).sum())
    assert np.isfinite(out["loss"]) and np.isfinite(out["kl"])


# ---- 8. guards
def test_guards(shipped):
    engine, ops, policy, value, rw = shipped
    own = torch.full((SLOTS,), START_OWN, dtype=torch.int64, device="cuda")
    opp = torch.full((SLOTS,), START_OPP, dtype=torch.int64, device="cuda")
    act = torch.ones(SLOTS, dtype=torch.uint8, device="cuda")
    for kw, what in ((dict(backup="reference"), "negamax"), (dict(selection="reference"), "alphazero"),
                     (dict(wave=8), "persistent search only")):
        m = _engine(shipped, **kw)
        before = m.tree.nodes.clone()
        e = engine.SelfPlayEngine(m)
        for call in (lambda: m.search(own, opp, act, 16, gumbel=GUMBEL), lambda: e.play(16, gumbel=GUMBEL),
                     lambda: e.play_stream(16, 12, gumbel=GUMBEL), lambda: e.play_match(16, gumbel=GUMBEL)):
            with pytest.raises(ValueError, match=what):
                call()
        assert torch.equal(m.tree.nodes, before)
        m.close()
    m = _engine(shipped)
    e = engine.SelfPlayEngine(m)
    for kw in (dict(root_noise=(77, 64)), dict(explore_turns=4), dict(root_noise=(77, 0), forced_playouts=512)):
        with pytest.raises(ValueError, match="gumbel is not available together"):
            e.play(16, gumbel=GUMBEL, **kw)
    with pytest.raises(ValueError, match="root_noise or forced_playouts"):
        m.search(own, opp, act, 16, gumbel=GUMBEL, root_noise=(77, 64))
    for bad in ((1, 256), (65, 256), (4, 0), (4, 256, 5000)):
        with pytest.raises(ValueError, match="gumbel"):
            m.search(own, opp, act, 16, gumbel=bad)
    with pytest.raises(ValueError, match="n_sims"):
        m.search(own, opp, act, 40000, gumbel=GUMBEL)
    with pytest.raises(ValueError, match="no search"):
        m.gumbel_move(act)
    # no whole-game launch; the library refuses it too, with real device arrays behind the arguments
    m.tree.reset()
    with pytest.raises(ValueError, match="not available with the Gumbel root search"):
        e._play_persistent(16, *e._start_boards(SLOTS), True, engine.PlayRules(None, 0, None, gumbel=GUMBEL + (50,)))
    st = m._gumbel_state()
    a, keep = m._search_args(own, opp, act, 16)
    a.max_turns = 60
    with pytest.raises(Exception, match="one search per launch"):
        ops.search_gumbel(a, GUMBEL + (50,), st["tables"], m._gumbel_sched(4, 16), st["g"])
    a, keep = m._search_args(own, opp, act, 16)
    a.games_per_workgroup &= ~0x200
    with pytest.raises(Exception, match="negamax"):
        ops.search_gumbel(a, GUMBEL + (50,), st["tables"], m._gumbel_sched(4, 16), st["g"])
    m.close()
    # the stream: the batch loop, with the record
    m = _engine(shipped)
    res = engine.SelfPlayEngine(m).play_stream(16, 12, gumbel=GUMBEL)
    assert res.launches == 2 and res.pi_raw.shape == res.pi.shape == (res.n_turns, 12, 64)
    assert int(res.pi_raw.sum()) == 15 * int((res.valid == 1).sum())
    m.close()
    # MCTS: one position
    from iago_amd import MCTS as M
    one = M.MCTS(n_thr=1, policy_net=policy, value_net=value, rollout_weights=rw, n_sims=16, capacity=4096, seed=SEED,
                 backup="negamax", selection="alphazero", gumbel=GUMBEL)
    assert one.get_move(orc.initial_state(), 1) in (19, 26, 37, 44)
    with pytest.raises(ValueError, match="n_sims"):
        M.MCTS(n_thr=1, policy_net=policy, value_net=value, rollout_weights=rw, backup="negamax", selection="alphazero",
               gumbel=GUMBEL)
    with pytest.raises(ValueError, match="negamax"):
        M.MCTS(n_thr=1, policy_net=policy, value_net=value, rollout_weights=rw, n_sims=16, gumbel=GUMBEL)
