"""Forced playouts and policy-target pruning on the GPU (SelfPlayEngine.play / play_stream(forced_playouts=k_256),
BatchedMCTS.search(forced_playouts=) / pruned_visits(); iago_mcts_search_forced, iago_mcts_prune_visits) against
tests/forced_ref.py, bit for bit: the pruning kernel alone on trees a noised, forced search wrote; the trees of one search
and of three consecutive turns against the oracle subclass fed the recorded z; whole games through the turn loop replayed
game by game.  Sizes: 8 slots (33 for the kernel's second workgroup), 24 playouts at n_thr 1 and 40 at n_thr 15, capacity
4096, random-init nets, the shipped rollout weights; (alpha_256, eps_256) = (77, 128), k_256 = 512."""
import numpy as np
import pytest
import torch

from oracle import mcts_py
from oracle import oracle as orc
from tests import explore_ref, forced_ref as fr, playout_cap_ref as cap_ref, root_noise_ref as rn
from tests.conftest import load_json
from tests.gpu_util import random_positions, state_of
from tests.test_oracle_golden import _cmp_tree

pytestmark = pytest.mark.gpu

SLOTS, N_SIMS, BASE, S0, SEED = 8, 24, 300, 1000, 11
NOISE, K256 = (77, 128), 512
CAP = (18, 64)
START_OWN, START_OPP = 0x0000000810000000, 0x0000001008000000


@pytest.fixture(scope="module")
def nets():
    from iago_amd import engine, network, ops
    assert torch.cuda.is_available()
    torch.manual_seed(3)
    policy = network.SLPolicy().cuda().eval()          # random init: broad trees
    value = network.Value().cuda().eval()
    g = load_json("simulate.json")
    return engine, ops, policy, value, ops.RolloutWeights(g["shipped_w"], g["shipped_b"])


@pytest.fixture(scope="module")
def probe(nets):
    from tests.test_mcts_production_gpu import NetProbe
    return NetProbe(nets[1], nets[2], nets[3])          # (memoised: the module's oracles share the nets' answers)


@pytest.fixture(scope="module")
def pool():
    """Reachable positions from the oracle's random games, by their number of legal moves."""
    own, opp = random_positions(400, seed=34)
    by_k = {}
    for o, p in zip(own, opp):
        by_k.setdefault(len(orc.legal_actions(state_of(o, p), 1)), []).append((int(o), int(p)))
    return by_k


def _engine(nets, slots=SLOTS, n_thr=1, base=BASE, **kw):
    engine, ops, policy, value, rw = nets
    kw.setdefault("persistent", True)
    kw.setdefault("capacity", 4096)
    m = engine.BatchedMCTS(slots, policy, value, rw, n_thr=n_thr, seed=SEED, game_id_base=base, **kw)
    m.sim_counter = S0
    return m


def _split_or_skip(m, split):
    if split and m._split is None:
        m.close()
        pytest.skip("this runtime gives no CU-masked streams")


def _oracle(probe, n_thr, game_id, noise=NOISE, k_256=K256):
    return fr.ForcedMCTS(probe.policy_fn, probe.value_fn, None, lmbda=0.5, c_puct=1.0, n_thr=n_thr,
                         noise=tuple(noise) + (rn.DRAWS,), seed=SEED, game_id=game_id, k_256=k_256)


def _root_children(d):
    """(action, n, P, Q) of the root's children from a TreePool.dump(): the device's float32 P and Q."""
    return [(a, d["children"][str(a)]["n"], np.float32(d["children"][str(a)]["P"]), np.float32(d["children"][str(a)]["Q"]))
            for a in d["order"]]


# ---- 1. iago_mcts_prune_visits alone, on the trees of a noised, forced search
@pytest.mark.parametrize("n_games", [8, 33])
def test_prune_visits_kernel_equals_prune_row(nets, pool, golden_rules, n_games):
    """One wave of 8-lane groups (8 games), and a second workgroup holding one game (33).  Game 0 .. 4: roots of 2, 8, 9, 16
    and 17 or more children (the select and the row walk take 8 and 16 children per step); 5: one child; 6: searched but
    left out of the pruning (inactive: its row is not touched); 7: a fresh root, no children; 32: alone in its workgroup."""
    engine, ops = nets[0], nets[1]
    wide = max(k for k in pool if k >= 17)
    pick = [pool[2][0], pool[8][0], pool[9][0], pool[16][0], pool[wide][0], pool[1][0], pool[8][1], pool[9][1]]
    rest = random_positions(n_games, seed=36)
    own = [p[0] for p in pick] + [int(x) for x in rest[0][8:]]
    opp = [p[1] for p in pick] + [int(x) for x in rest[1][8:]]
    if n_games > 32:
        own[32], opp[32] = pool[16][1]
        eb = golden_rules["edge_boards"]
        own[9], opp[9] = eb[6][0], eb[6][1]      # 'pass1': the mover must pass -- a pass child, an empty row
    acts = [orc.legal_actions(state_of(own[g], opp[g]), 1) for g in range(n_games)]
    assert [len(a) for a in acts[:6]] == [2, 8, 9, 16, wide, 1] and wide >= 17
    m = _engine(nets, slots=n_games)
    o, p = ops.bits_to_tensor(own), ops.bits_to_tensor(opp)
    searched = torch.ones(n_games, dtype=torch.uint8, device="cuda")
    searched[7] = 0
    m.tree.reset()
    m.search(o, p, searched, 40, root_noise=NOISE, turn=0, forced_playouts=K256)
    live = torch.ones(n_games, dtype=torch.uint8, device="cuda")
    live[6] = 0
    nodes_before = m.tree.nodes.cpu().numpy().copy()
    raw = m.best_move(None)[1].cpu().numpy().copy()
    reduced = 0
    for k_256 in (K256, 4096, 1):
        rows = torch.full((n_games, 64), 0x77777, dtype=torch.int32, device="cuda")
        assert ops.prune_visits(m.tree.ref(), live, m.c_puct, k_256, rows) is rows
        got = rows.cpu().numpy()
        for g in range(n_games):
            if g == 6:
                assert np.all(got[g] == 0x77777), g
                continue
            d = m.tree.dump(g, max_depth=1)
            ch = _root_children(d)
            want = fr.prune_row(ch, d["n"], 1.0, k_256)
            assert np.array_equal(got[g], want), (g, k_256, got[g][got[g] != want], want[got[g] != want])
            assert np.all(got[g] <= raw[g])
            if g == 7:
                assert not ch and not got[g].any()
            elif len(acts[g]) < 2:
                assert len(ch) == 1 and np.array_equal(got[g], raw[g]), g
                assert (ch[0][0] == -1 and not got[g].any()) if not acts[g] else got[g][acts[g][0]] == ch[0][1]
            else:
                assert [c[0] for c in ch] == acts[g], g
                reduced += int(got[g].sum()) < int(raw[g].sum()) and k_256 == K256
    assert reduced >= 2                                           # (rows the kernel pruned, at the games' own k)
    # the engine's call, the same rows; the trees were only read
    got = m.pruned_visits(live, K256).cpu().numpy()
    want = torch.full((n_games, 64), 0, dtype=torch.int32, device="cuda")
    ops.prune_visits(m.tree.ref(), live, m.c_puct, K256, want)
    keep = np.arange(n_games) != 6
    assert np.array_equal(got[keep], want.cpu().numpy()[keep])
    assert np.array_equal(m.tree.nodes.cpu().numpy(), nodes_before)
    m.close()


# ---- 2. / 3. the search: trees and pruned rows against the oracle subclass, z replayed
def _run_turns(nets, probe, own, opp, n_thr, n_sims, noise, turns, split, base=BASE):
    """`turns` consecutive searched turns of the games (own, opp) on the device and in the oracle subclass, compared
    after every turn: the whole tree and the pruned row.  Returns (selections a forced child won, roots that had their
    children at a turn's start, rows pruned)."""
    engine, ops = nets[0], nets[1]
    G = len(own)
    m = _engine(nets, slots=G, n_thr=n_thr, base=base, z_log_rows=n_sims, **(dict(split=8) if split else {}))
    _split_or_skip(m, split)
    oms = [_oracle(probe, n_thr, base + g, noise) for g in range(G)]
    states, colors = [state_of(own[g], opp[g]) for g in range(G)], [1] * G
    o, p = ops.bits_to_tensor(own), ops.bits_to_tensor(opp)
    reused = pruned = 0
    m.tree.reset()
    for t in range(turns):
        acts = [orc.legal_actions(states[g], colors[g]) for g in range(G)]
        active = torch.tensor([1 if a else 0 for a in acts], dtype=torch.uint8, device="cuda")
        m.z_log_n.zero_()
        m.search(o, p, active, n_sims, root_noise=noise, turn=t, forced_playouts=K256)
        zlog = m.z_log.cpu().numpy()
        move = m.best_move(active)[0].cpu().numpy().copy()
        raw = m.visits.cpu().numpy().copy()
        rows = m.pruned_visits(active, K256).cpu().numpy()
        for g in range(G):
            om = oms[g]
            if not acts[g]:
                move[g] = -1
                om.update_with_move(-1)
                continue
            it = iter(zlog[:n_sims, g])
            om.rollout_fn = lambda s, c, it=it: int(next(it))
            reused += len(om.root.children) >= 2
            om.begin_turn(states[g], colors[g], t)
            want = om.get_move(states[g], colors[g], n_sims)
            assert next(it, None) is None
            _cmp_tree(m.tree.dump(g, max_depth=64), mcts_py.dump_tree(om.root, max_depth=64), "g%d t%d" % (g, t))
            # (the root's children's P to the bit: the rule reads them)
            got_p = [c[2] for c in _root_children(m.tree.dump(g, max_depth=1))]
            assert [np.float32(x).tobytes() for x in got_p] == [np.float32(ch.P).tobytes() for ch in om.root.children.values()]
            assert move[g] == want, (g, t)
            assert np.array_equal(raw[g], fr.raw_row(om.root)), (g, t)
            assert np.array_equal(rows[g], om.pruned_row()), (g, t, rows[g], om.pruned_row())
            pruned += int(rows[g].sum()) < int(raw[g].sum())
            om.update_with_move(int(want))
            orc.place_stone(states[g], int(want), colors[g])
        mv = torch.from_numpy(move.astype(np.int8)).cuda()
        m.update_with_move(mv, torch.ones(G, dtype=torch.uint8, device="cuda"))
        ops.apply_moves(o, p, mv)
        o, p = p, o
        colors = [3 - c for c in colors]
    m.close()
    return sum(om.n_forced for om in oms), reused, pruned


@pytest.mark.parametrize("split", [False, True], ids=["single", "split"])
@pytest.mark.parametrize("eps", [128, 0])
@pytest.mark.parametrize("n_thr,n_sims", [(15, 40), (1, 24)])
def test_one_forced_search_bit_exact_vs_the_oracle_subclass(nets, probe, pool, n_thr, n_sims, eps, split):
    """Four games from the start position (ids alone differ) and four from a mid-game position of an oracle game with 17
    or more legal moves.  n_thr 15: the root expands inside the search (forcing starts with the children); n_thr 1: deep
    trees -- a forcing that leaked below the root would show in any of their nodes."""
    wide = pool[max(k for k in pool if k >= 17)][0]
    own = [START_OWN] * 4 + [wide[0]] * 4
    opp = [START_OPP] * 4 + [wide[1]] * 4
    forced, _, pruned = _run_turns(nets, probe, own, opp, n_thr, n_sims, (NOISE[0], eps), 1, split)
    print("n_thr %d eps %d: selections a forced child won %d, rows pruned %d of 8" % (n_thr, eps, forced, pruned))
    assert forced > 0 and pruned > 0


def test_a_reused_root_three_turns(nets, probe):
    """Three consecutive turns with update_with_move between them: from turn 1 on the root carries its N and its
    children's n from the turn before, and the rule reads them as they are."""
    forced, reused, pruned = _run_turns(nets, probe, [START_OWN] * 8, [START_OPP] * 8, 1, N_SIMS, NOISE, 3, False, base=BASE + 40)
    assert forced > 0 and reused >= 8 and pruned > 0


# ---- 4. whole games through the turn loop
RECORDS = ("own", "opp", "valid", "move", "pi", "pi_raw", "z", "final_p1", "final_p2")
GAMES = {"forced": dict(n_thr=1, kw=dict(explore_turns=4)),
         "cap": dict(n_thr=15, kw=dict(explore_turns=4, playout_cap=CAP)),
         "solve": dict(n_thr=1, kw=dict(explore_turns=4, solve_empties=6))}


@pytest.fixture(scope="module")
def games(nets):
    out = {}
    for name, spec in GAMES.items():
        m = _engine(nets, n_thr=spec["n_thr"], z_log_rows=128 * N_SIMS)
        res = nets[0].SelfPlayEngine(m).play(N_SIMS, root_noise=NOISE, forced_playouts=K256, **spec["kw"])
        s = {k: getattr(res, k).cpu().numpy() for k in RECORDS}
        s.update(n_turns=res.n_turns, launches=res.launches, base=res.game_id_base, res=res,
                 zlog=m.z_log.cpu().numpy(), zn=m.z_log_n.cpu().numpy())
        m.close()
        out[name] = s
    return out


def _replay(probe, s, g, n_thr, explore_turns=4, capped=False, solved_from=None):
    """Game g of a batch replayed by the oracle subclass from the searches' z record: move, pi, pi_raw and valid of every
    turn.  Under the cap a fast turn has n_fast playouts, clean priors, no forcing and pi = pi_raw."""
    it = iter(s["zlog"][:s["zn"][g], g])
    om = _oracle(probe, n_thr, s["base"] + g)
    om.rollout_fn = lambda st, c: int(next(it))
    state = orc.initial_state()
    stone_num, pass_flg, t, kinds = 4, False, 0, set()
    while stone_num < 64:
        for color in (1, 2):
            acts = orc.legal_actions(state, color)
            if len(acts) > 0:
                if s["valid"][t, g] == 3:
                    assert solved_from is not None and int((np.asarray(state) == 0).sum()) <= solved_from, (g, t)
                    assert not s["pi"][t, g].any() and not s["pi_raw"][t, g].any(), (g, t)
                    a = int(s["move"][t, g])
                    assert a in acts, (g, t)
                    kinds.add("solved")
                else:
                    full = not capped or cap_ref.is_full(SEED, s["base"] + g, t, CAP[1])
                    om.begin_turn(state, color, t, noised=full)
                    best = om.get_move(state, color, N_SIMS if full else CAP[0])
                    raw = fr.raw_row(om.root)
                    a = explore_ref.draw(raw, SEED, s["base"] + g, t) if t < explore_turns else best
                    assert s["valid"][t, g] == (1 if full else 4), (g, t)
                    assert np.array_equal(s["pi_raw"][t, g], raw), (g, t)
                    assert np.array_equal(s["pi"][t, g], om.pruned_row() if full else raw), (g, t)
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
    return kinds


@pytest.mark.parametrize("g", range(SLOTS))
def test_whole_forced_games_replayed_by_the_oracle_subclass(probe, games, g):
    s = games["forced"]
    assert s["launches"] == s["n_turns"] > 1     # (the turn loop)
    assert _replay(probe, s, g, 1) == {True}


@pytest.mark.parametrize("name", list(GAMES))
def test_pruned_rows_lie_under_the_raw_rows(games, name):
    s = games[name]
    assert s["pi"].shape == s["pi_raw"].shape and s["pi"].dtype == s["pi_raw"].dtype == np.int32
    assert np.all(s["pi"] <= s["pi_raw"]) and np.all(s["pi"] >= 0)
    less = s["pi"].sum(axis=2) < s["pi_raw"].sum(axis=2)
    print(name, "rows pruned:", int(less.sum()), "of", int((s["valid"] == 1).sum()), "forced rows")
    assert not less[s["valid"] != 1].any()                         # on forced (valid 1) rows only
    assert less.any() or name == "cap"     # (the CPU run shows the reference prunes at these parameters; few full turns under the cap)
    assert np.array_equal(s["pi"].argmax(axis=2)[s["valid"] == 1], s["pi_raw"].argmax(axis=2)[s["valid"] == 1])
    # the move comes from the raw counts: from explore_turns on it is their first maximum
    late = (s["valid"] == 1) & (np.arange(s["valid"].shape[0]).reshape(-1, 1) >= 4)
    assert np.array_equal(s["move"][late], s["pi_raw"].argmax(axis=2)[late])


def test_under_a_playout_cap_only_the_full_turns_are_forced_and_pruned(probe, games):
    s = games["cap"]
    fast = s["valid"] == 4
    assert fast.any() and (s["valid"] == 1).any()
    assert np.array_equal(s["pi"][fast], s["pi_raw"][fast])          # fast rows: pi == pi_raw
    assert np.all(s["pi_raw"][fast].sum(axis=1) >= CAP[0] - 15)
    assert _replay(probe, s, 2, 15, capped=True) == {True, False}


def test_composed_with_the_endgame_solver(probe, games):
    s = games["solve"]
    assert (s["valid"] == 3).any()
    assert _replay(probe, s, 5, 1, solved_from=6) == {True, "solved"}


# ---- 5. forced_playouts=None is the parent's call
def test_none_is_the_noised_play_of_before(nets, monkeypatch):
    from iago_amd import engine, ops

    def host(r):
        return {k: getattr(r, k).cpu().numpy() for k in RECORDS if k != "pi_raw"}
    m = _engine(nets)
    want_res = engine.SelfPlayEngine(m).play(N_SIMS, root_noise=NOISE, explore_turns=4)
    want = host(want_res)
    m.close()

    def never(*a, **k):
        raise AssertionError("forced_playouts = None reached the forced playouts' entry points")
    monkeypatch.setattr(ops, "search_forced", never)
    monkeypatch.setattr(ops, "prune_visits", never)
    searches = []
    real_search = engine.BatchedMCTS.search

    def spy_search(self, *a, **k):
        searches.append((len(a), sorted(k)))
        return real_search(self, *a, **k)
    monkeypatch.setattr(engine.BatchedMCTS, "search", spy_search)
    m = _engine(nets)
    res = engine.SelfPlayEngine(m).play(N_SIMS, root_noise=NOISE, explore_turns=4, forced_playouts=None)
    m.close()
    got = host(res)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    # (today's calls, argument for argument; and the attribute existing readers may meet: None, on every result)
    assert searches and all(x == (4, ["check", "counts", "root_noise", "turn"]) for x in searches)
    assert res.pi_raw is None and want_res.pi_raw is None and "pi_raw" not in res.tuples()


# ---- 6. training on the pruned targets
def test_the_trainer_steps_on_the_pruned_rows(nets, games, monkeypatch):
    from iago_amd import network
    from iago_amd.train_rl import ReinforceTrainer
    s = games["forced"]
    model = network.SLPolicy()
    model.load_state_dict(nets[2].state_dict())
    tr = ReinforceTrainer(model, pool_dir=None, N=2, seed=1)
    seen = []
    real = tr._update_visits

    def spy(own, opp, pi):
        seen.append(pi.sum(dim=1).cpu().numpy().copy())
        return real(own, opp, pi)
    monkeypatch.setattr(tr, "_update_visits", spy)
    tup = s["res"].tuples()
    out = tr.step_from_tuples(tup, target="visits")
    searched = s["valid"] == 1
    assert out["n_tuples"] == int(searched.sum()) and np.isfinite(out["loss"])
    # the targets are the pruned rows: the canonical order is (turn, game), the records' own
    assert len(seen) == 1 and np.array_equal(seen[0], s["pi"].sum(axis=2)[searched])
    assert not np.array_equal(seen[0], s["pi_raw"].sum(axis=2)[searched])


# ---- 7. guards
def test_guards(nets):
    engine, ops, policy, value, rw = nets
    m = _engine(nets)
    e = engine.SelfPlayEngine(m)
    own = torch.full((SLOTS,), START_OWN, dtype=torch.int64, device="cuda")
    opp = torch.full((SLOTS,), START_OPP, dtype=torch.int64, device="cuda")
    act = torch.ones(SLOTS, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="requires root_noise"):
        e.play(N_SIMS, forced_playouts=K256)
    with pytest.raises(ValueError, match="requires root_noise"):
        e.play_stream(N_SIMS, 16, forced_playouts=K256)
    with pytest.raises(ValueError, match="requires root_noise"):
        m.search(own, opp, act, N_SIMS, forced_playouts=K256)
    for bad in (0, 4097, 2.0, True):
        with pytest.raises(ValueError, match="forced_playouts"):
            e.play(N_SIMS, root_noise=NOISE, forced_playouts=bad)
        with pytest.raises(ValueError, match="forced_playouts"):
            m.search(own, opp, act, N_SIMS, root_noise=NOISE, forced_playouts=bad)
        with pytest.raises(ValueError, match="forced_playouts"):
            m.pruned_visits(act, bad)
    with pytest.raises(ValueError, match="forced_playouts is not available"):
        e.play_match(N_SIMS, forced_playouts=K256)
    # no whole-game launch, as for the noise alone
    m.tree.reset()
    with pytest.raises(ValueError, match="not available with root noise"):
        e._play_persistent(N_SIMS, *e._start_boards(SLOTS), True, engine.PlayRules(None, 0, None, NOISE + (256,), K256))
    m.close()
    # the stream: the batch loop, with the record
    m = _engine(nets)
    res = engine.SelfPlayEngine(m).play_stream(N_SIMS, 12, root_noise=NOISE, forced_playouts=K256)
    assert res.launches == 2 and res.pi_raw.shape == res.pi.shape == (res.n_turns, 12, 64)
    assert bool((res.pi <= res.pi_raw).all()) and int(res.pi.sum()) < int(res.pi_raw.sum())
    m.close()
