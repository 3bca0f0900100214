"""Root noise on the GPU (SelfPlayEngine.play / play_stream(root_noise=(alpha_256, eps_256[, draws])),
BatchedMCTS.search(root_noise=); iago_mcts_root_noise, iago_mcts_search_noise) against tests/root_noise_ref.py: the urn's
counts and the mixed priors bit for bit, the trees of a search against the oracle subclass fed the recorded z, and whole
games, which run through the turn loop (root noise has no whole-game launch): the single launch per turn, the role split
and play_stream play the same games, record for record, and two games are rebuilt by the oracle subclass.  Sizes of
test_explore_gpu.py: 64 slots, 24 playouts, n_thr 15, capacity 4096, random-init nets, the shipped rollout weights.

The playout cap composed here is (18, 64), test_playout_cap_gpu.py's: at n_thr 15 a fast turn of 6 playouts leaves a fresh
root without children, which the engine refuses with or without noise (test_a_cap_of_6_needs_n_thr_1); the cap (6, 64) is
played with the noise at n_thr 1, where a root expands at its second playout."""
import numpy as np
import pytest
import torch

from oracle import mcts_py
from oracle import oracle as orc
from tests import explore_ref, playout_cap_ref as cap_ref, root_noise_ref as rn
from tests.conftest import load_json
from tests.gpu_util import random_positions, state_of
from tests.test_oracle_golden import _cmp_tree

pytestmark = pytest.mark.gpu

SLOTS, N_GAMES, N_SIMS, BASE, S0, SEED, N_THR = 64, 160, 24, 300, 1000, 11, 15
NOISE = (77, 64)
CAP = (18, 64)
RECORDS = ("own", "opp", "valid", "move", "pi", "z", "final_p1", "final_p2")
VARIANTS = {"noise": {}, "all": dict(explore_turns=8, solve_empties=8, playout_cap=CAP)}
WRAP = 0xFFFFFFF0   # game ids that wrap around 2^32


@pytest.fixture(scope="module")
def nets():
    from iago_amd import engine, network, ops
    assert torch.cuda.is_available()
    torch.manual_seed(3)
    policy = network.SLPolicy().cuda().eval()          # random init: broad trees
    value = network.Value().cuda().eval()
    g = load_json("simulate.json")
    return engine, ops, policy, value, ops.RolloutWeights(g["shipped_w"], g["shipped_b"])


def _engine(nets, base=BASE, slots=SLOTS, n_thr=N_THR, **kw):
    engine, ops, policy, value, rw = nets
    kw.setdefault("persistent", True)
    kw.setdefault("capacity", 4096)
    m = engine.BatchedMCTS(slots, policy, value, rw, n_thr=n_thr, seed=SEED, game_id_base=base, **kw)
    m.sim_counter = S0
    return m


def _host(r):
    out = {k: getattr(r, k).cpu().numpy() for k in RECORDS}
    out["game_turns"] = r.game_turns.cpu().numpy() if r.game_turns is not None else None
    out["n_turns"], out["launches"], out["base"] = r.n_turns, r.launches, r.game_id_base
    return out


def _play(nets, base=BASE, engine_kw=None, **kw):
    m = _engine(nets, base=base, **(engine_kw or {}))
    if (engine_kw or {}).get("split") and m._split is None:
        m.close()
        pytest.skip("this runtime gives no CU-masked streams")
    out = _host(nets[0].SelfPlayEngine(m).play(N_SIMS, **kw))
    out["sim"], out["split"], out["evals"] = m.sim_counter, m._split is not None, m.n_leaf_evals
    m.close()
    return out


def _same(a, b, keys=RECORDS + ("n_turns", "sim")):
    for k in keys:
        assert np.array_equal(a[k], b[k]), k


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


# ---- 1. the kernel: counts rows and the children's priors against the reference
WIDE_OWN = sum(1 << a for a in (27, 28, 35, 36))
WIDE_OPP = sum(1 << (8 * r + c) for r in range(2, 6) for c in range(2, 6)) & ~WIDE_OWN


def _kernel_positions(golden_rules):
    """64 roots: random reachable positions, with a pass (K = 0), a dead board (K = 0), K = 1, K = 2 and a hand-made one
    with 20 legal moves (the centre four in a ring of twelve) among them."""
    own, opp = random_positions(SLOTS, seed=33)
    pool = random_positions(400, seed=34)
    ks = [len(orc.legal_actions(state_of(o, p), 1)) for o, p in zip(*pool)]
    eb = golden_rules["edge_boards"]
    own[1], opp[1] = eb[6][0], eb[6][1]       # 'pass1': the mover must pass
    own[2], opp[2] = eb[5][0], eb[5][1]       # 'dead': nobody can move
    for g, k in ((5, 1), (6, 2), (7, 1), (8, 2)):
        i = ks.index(k)
        ks[i] = -1
        own[g], opp[g] = pool[0][i], pool[1][i]
    for g in (10, 11):
        own[g], opp[g] = WIDE_OWN, WIDE_OPP
    return own, opp


@pytest.mark.parametrize("draws", [16, 1024])
def test_root_noise_kernel_equals_the_reference(nets, golden_rules, draws):
    engine, ops = nets[0], nets[1]
    own, opp = _kernel_positions(golden_rules)
    acts = [orc.legal_actions(state_of(own[g], opp[g]), 1) for g in range(SLOTS)]
    assert len(acts[1]) == 0 and len(acts[2]) == 0 and len(acts[5]) == 1 and len(acts[6]) == 2 and len(acts[10]) >= 20
    m = _engine(nets, base=WRAP)
    cap = m.tree.capacity
    o, p = ops.bits_to_tensor(own), ops.bits_to_tensor(opp)
    searched = torch.ones(SLOTS, dtype=torch.uint8, device="cuda")
    searched[3::4] = 0                       # (these keep a fresh root: a counts row, no child to rewrite)
    searched[7] = 1                          # (a K = 1 root with its single child; 11, a wide one, stays fresh)
    m.tree.reset()
    m.search(o, p, searched, N_SIMS)         # plain: the searched roots have their children, clean
    live = torch.ones(SLOTS, dtype=torch.uint8, device="cuda")
    for g in (4, 9, 12, 63):
        live[g] = 0
    ids = ((torch.arange(SLOTS, dtype=torch.int64) + WRAP) & 0xFFFFFFFF)
    assert int(ids[15]) == 0xFFFFFFFF and int(ids[16]) == 0
    ids32 = torch.where(ids >= (1 << 31), ids - (1 << 32), ids).to(torch.int32).cuda()
    root = m.tree.root.cpu().numpy()
    fc = m.tree.first_child.cpu().numpy()
    nch = m.tree.n_children.cpu().numpy()
    nodes_before = m.tree.nodes.cpu().numpy().copy()
    expect = m.tree.p.cpu().numpy().copy()
    rewritten = fresh = 0
    for rep in range(3):                     # several turns: every game's turn moves on, the mix compounds
        turns = (torch.arange(SLOTS, dtype=torch.int32) * 3 + rep) % 7
        counts = torch.full((SLOTS, 64), 0x7777, dtype=torch.int16, device="cuda")
        out = ops.root_noise(m.tree.ref(), live, o, p, SEED, ids32, turns.cuda(), NOISE + (draws,), counts)
        assert out is counts
        got = counts.cpu().numpy()
        for g in range(SLOTS):
            if not int(live[g]):
                assert np.all(got[g] == 0x7777), g
                continue
            want = rn.counts(acts[g], SEED, int(ids[g]), int(turns[g]), NOISE[0], draws)
            assert np.array_equal(got[g], want), (g, rep, got[g][got[g] != want], want[got[g] != want])
            assert int(want.sum()) == (draws if len(acts[g]) >= 2 else 0)
            at = g * cap + int(root[g])
            if fc[at] >= 0 and len(acts[g]) >= 2:
                assert nch[at] == len(acts[g])
                for j, a in enumerate(acts[g]):
                    i = g * cap + int(fc[at]) + j
                    expect[i] = rn.mix(expect[i], want[a], NOISE[1], draws)
                rewritten += 1
            elif len(acts[g]) >= 2:
                fresh += 1
        now = m.tree.p.cpu().numpy()
        assert np.array_equal(_bits(now), _bits(expect)), np.nonzero(_bits(now) != _bits(expect))[0][:8]
    assert rewritten >= 3 * 30 and fresh >= 3 * 8
    # nothing but the priors moved: every other field of every node, the roots, the pools
    after = m.tree.nodes.cpu().numpy().copy()
    after.reshape(-1, 8)[:, 2] = nodes_before.reshape(-1, 8)[:, 2]
    assert np.array_equal(after, nodes_before)
    assert np.array_equal(m.tree.root.cpu().numpy(), root)
    # the engine's own call: BatchedMCTS.search(root_noise=) with every game inactive touches nothing
    m.search(o, p, torch.zeros(SLOTS, dtype=torch.uint8, device="cuda"), N_SIMS, root_noise=NOISE, turn=0)
    assert np.array_equal(_bits(m.tree.p.cpu().numpy()), _bits(expect))
    m.close()


# ---- 2. one search: the trees against the oracle subclass, z replayed (tests/test_mcts_production_gpu.py)
@pytest.mark.parametrize("n_thr", [15, 1])
def test_noised_search_trees_bit_exact_vs_the_oracle_subclass(nets, n_thr):
    from tests.test_mcts_production_gpu import NetProbe
    engine, ops, policy, value, rw = nets
    G, TURNS, noise = 8, 5, NOISE + (64,)
    own, opp = random_positions(G, seed=35)
    own[:4], opp[:4] = 0x0000000810000000, 0x0000001008000000        # four games from the opening: ids alone differ
    m = _engine(nets, base=WRAP + 12, slots=G, n_thr=n_thr, z_log_rows=N_SIMS)
    probe = NetProbe(ops, policy, value)
    oms, states, colors = [], [], []
    for g in range(G):
        oms.append(rn.NoisyMCTS(probe.policy_fn, probe.value_fn, None, lmbda=0.5, c_puct=1.0, n_thr=n_thr, noise=noise,
                                seed=SEED, game_id=WRAP + 12 + g))
        states.append(state_of(own[g], opp[g]))
        colors.append(1)
    o, p = ops.bits_to_tensor(own), ops.bits_to_tensor(opp)
    at_start = in_search = 0
    m.tree.reset()
    for t in range(TURNS):
        acts = [orc.legal_actions(states[g], colors[g]) for g in range(G)]
        active = torch.tensor([1 if a else 0 for a in acts], dtype=torch.uint8, device="cuda")
        m.z_log_n.zero_()
        m.search(o, p, active, N_SIMS, root_noise=noise, turn=t)
        zlog = m.z_log.cpu().numpy()
        move = m.best_move(active)[0].cpu().numpy().copy()
        for g in range(G):
            om = oms[g]
            if not acts[g]:
                move[g] = -1
                om.update_with_move(-1)
                continue
            it = iter(zlog[:N_SIMS, g])
            om.rollout_fn = lambda s, c, it=it: int(next(it))
            had = len(om.root.children) >= 2
            before = len(om.mixed)
            om.begin_turn(states[g], colors[g], t)
            want = om.get_move(states[g], colors[g], N_SIMS)
            assert next(it, None) is None
            if len(acts[g]) >= 2:
                assert len(om.mixed) - before == len(acts[g]), (g, t)      # mixed once: at the start or in the search
                at_start += had
                in_search += not had
            _cmp_tree(m.tree.dump(g, max_depth=64), mcts_py.dump_tree(om.root, max_depth=64), "g%d t%d" % (g, t))
            assert move[g] == want, (g, t)
            om.update_with_move(int(want))
            orc.place_stone(states[g], int(want), colors[g])
        mv = torch.from_numpy(move.astype(np.int8)).cuda()
        m.update_with_move(mv, torch.ones(G, dtype=torch.uint8, device="cuda"))
        ops.apply_moves(o, p, mv)
        o, p = p, o
        colors = [3 - c for c in colors]
    print("n_thr %d: roots mixed at the turn's start %d, in the search %d" % (n_thr, at_start, in_search))
    assert in_search > 0 and (n_thr == 15 or at_start > 0)
    m.close()


# ---- 3. whole games
@pytest.fixture(scope="module")
def plain(nets):
    return _play(nets)


@pytest.fixture(scope="module")
def noised(nets):
    return {k: _play(nets, root_noise=NOISE, **kw) for k, kw in VARIANTS.items()}


def _check_rules(s, explore_turns=0, solved_from=None, capped=False):
    """test_playout_cap_gpu._check_rules: the records are games by the rules -- the recorded position, a search or a
    pass by the mover's legal set, the move the visit row's first maximum (below explore_turns the reference's draw),
    valid 1 / 4 by the cap's reference, the books, the result and the final board."""
    own, opp = s["own"].view(np.uint64), s["opp"].view(np.uint64)
    p1s, p2s = s["final_p1"].view(np.uint64), s["final_p2"].view(np.uint64)
    for G in range(s["valid"].shape[1]):
        state = orc.initial_state()
        stone_num, pass_flg, t, over = 4, False, 0, False
        while not over and t < 128:
            for color in (1, 2):
                p1, p2 = orc.state_to_bits(state)
                mover = (p1, p2) if color == 1 else (p2, p1)
                assert (int(own[t, G]), int(opp[t, G])) == mover, (G, t)
                acts = orc.legal_actions(state, color)
                row = s["pi"][t, G]
                if len(acts) > 0:
                    a = int(s["move"][t, G])
                    assert a in acts, (G, t, a)
                    if s["valid"][t, G] == 3:
                        assert solved_from is not None and 64 - bin(p1 | p2).count("1") <= solved_from, (G, t)
                        assert not row.any(), (G, t)
                    else:
                        code = cap_ref.valid_code(SEED, s["base"] + G, t, CAP[1]) if capped else 1
                        assert s["valid"][t, G] == code, (G, t)
                        assert np.all(row[[x for x in range(64) if x not in acts]] == 0), (G, t)
                        n = N_SIMS if code == 1 else CAP[0]
                        assert row[a] > 0 and int(row.sum()) >= n - N_THR, (G, t)
                        want = explore_ref.draw(row, SEED, s["base"] + G, t) if t < explore_turns else int(np.argmax(row))
                        assert a == want, (G, t, a, want)
                    orc.place_stone(state, a, color)
                    stone_num += 1
                    pass_flg = False
                else:
                    assert s["valid"][t, G] == 0 and s["move"][t, G] == -1 and not row.any(), (G, t)
                    if pass_flg:
                        stone_num = 64
                    pass_flg = True
                t += 1
            if stone_num >= 64:
                over = True
        assert over and t % 2 == 0, (G, t)
        if s["game_turns"] is not None:
            assert int(s["game_turns"][G]) == t, (G, t)
        assert s["z"][G] == orc.judge(state, 1), G
        assert orc.state_to_bits(state) == (int(p1s[G]), int(p2s[G])), G


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_noised_games_follow_the_rules_and_differ_from_plain(noised, plain, variant):
    s = noised[variant]
    assert s["launches"] == s["n_turns"] > 1          # (the turn loop, whatever the engine could do in one launch)
    _check_rules(s, explore_turns=8 if variant == "all" else 0, solved_from=8 if variant == "all" else None,
                 capped=variant == "all")
    t = min(s["n_turns"], plain["n_turns"])
    assert s["n_turns"] != plain["n_turns"] or any(not np.array_equal(s[k][:t], plain[k][:t]) for k in ("move", "pi"))
    if variant == "noise":
        # the noise moves visits at turn 0 already: the same roots, nets and rollout streams as the plain games'
        assert not np.array_equal(s["pi"][0], plain["pi"][0])
        assert np.all(s["pi"][0].sum(axis=1) == N_SIMS - N_THR)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_role_split_plays_the_same_games(nets, noised, variant):
    s = _play(nets, engine_kw=dict(split=8), root_noise=NOISE, **VARIANTS[variant])   # (skips without CU-masked streams)
    assert s["split"] and s["launches"] == noised[variant]["launches"]
    _same(s, noised[variant])


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_stream_equals_the_batch_loop(nets, noised, variant):
    kw = VARIANTS[variant]
    parts = [noised[variant]] + [_play(nets, base=BASE + k * SLOTS, root_noise=NOISE, **kw) for k in (1, 2)]
    m = _engine(nets)
    s = _host(nets[0].SelfPlayEngine(m).play_stream(N_SIMS, N_GAMES, root_noise=NOISE, **kw))
    sim, ctl3 = m.sim_counter, int(m._ps["ctl"][3].item())
    m.close()
    assert s["launches"] == 3 and ctl3 == 0 and s["valid"].shape[1] == N_GAMES       # (the batch loop: three batches)
    for G in range(N_GAMES):
        b, c = parts[G // SLOTS], G % SLOTS
        t = int(s["game_turns"][G])
        assert t <= b["n_turns"] and not b["valid"][t:, c].any(), G
        for k in ("z", "final_p1", "final_p2"):
            assert s[k][G] == b[k][c], (G, k)
        for k in ("own", "opp", "valid", "move", "pi"):
            assert np.array_equal(s[k][:t, G], b[k][:t, c]), (G, k)
    assert s["n_turns"] == int(s["game_turns"].max())
    assert sim == (S0 + s["n_turns"] * N_SIMS) & 0xFFFFFFFF


def _rebuild(nets, m, res, g, capped):
    """Game g of a batch rebuilt by the oracle subclass from the searches' z record: move for move, visit row for visit
    row; under the cap a fast turn has n_fast playouts and CLEAN priors."""
    from tests.test_mcts_production_gpu import NetProbe
    engine, ops, policy, value, rw = nets
    moves, valid, pi = res.move.cpu().numpy(), res.valid.cpu().numpy(), res.pi.cpu().numpy()
    zlog, zn = m.z_log.cpu().numpy(), m.z_log_n.cpu().numpy()
    it = iter(zlog[:zn[g], g])
    probe = NetProbe(ops, policy, value)
    om = rn.NoisyMCTS(probe.policy_fn, probe.value_fn, lambda s, c: int(next(it)), lmbda=0.5, c_puct=1.0, n_thr=N_THR,
                      noise=NOISE + (rn.DRAWS,), seed=SEED, game_id=res.game_id_base + g)
    state = orc.initial_state()
    stone_num, pass_flg, t, kinds = 4, False, 0, set()
    while stone_num < 64:
        for color in (1, 2):
            acts = orc.legal_actions(state, color)
            if len(acts) > 0:
                full = not capped or cap_ref.is_full(SEED, res.game_id_base + g, t, CAP[1])
                om.begin_turn(state, color, t, noised=full)
                a = om.get_move(state, color, N_SIMS if full else CAP[0])
                row = np.zeros(64, np.int64)
                for b, ch in om.root.children.items():
                    row[b] = ch.n_visits
                assert valid[t, g] == (1 if full else 4), (g, t)
                assert np.array_equal(pi[t, g], row), (g, t)
                assert moves[t, g] == a, (g, t)
                kinds.add(full)
                om.update_with_move(a)
                orc.place_stone(state, a, color)
                stone_num += 1
                pass_flg = False
            else:
                assert valid[t, g] == 0 and moves[t, g] == -1, (g, t)
                if pass_flg:
                    stone_num = 64
                pass_flg = True
                om.update_with_move(-1)
            t += 1
    assert next(it, None) is None, g             # the oracle consumed exactly the playouts the launch ran
    assert res.z.cpu().numpy()[g] == orc.judge(state, 1), g
    return kinds


def test_two_whole_games_rebuilt_by_the_oracle_subclass(nets):
    for capped, g in ((False, 3), (True, 5)):
        m = _engine(nets, slots=8, z_log_rows=128 * N_SIMS)
        res = nets[0].SelfPlayEngine(m).play(N_SIMS, root_noise=NOISE, **(dict(playout_cap=CAP) if capped else {}))
        assert res.launches == res.n_turns
        kinds = _rebuild(nets, m, res, g, capped)
        assert kinds == ({True, False} if capped else {True})      # (the capped game has clean fast turns and noised full ones)
        m.close()


def test_eps_0_is_the_plain_engine(nets, plain):
    s = _play(nets, root_noise=(NOISE[0], 0))
    assert s["launches"] == s["n_turns"] and plain["launches"] == 1      # (the turn loop against the plain one launch)
    _same(s, plain)
    assert s["evals"] == plain["evals"]


def test_none_is_todays_play(nets, plain, monkeypatch):
    from iago_amd import engine, ops

    def never(*a, **k):
        raise AssertionError("root_noise = None reached the root noise's entry points")
    monkeypatch.setattr(ops, "search_noise", never)
    monkeypatch.setattr(ops, "root_noise", never)
    launches, searches = [], []
    real_launch, real_search = engine.BatchedMCTS._launch_persistent, engine.BatchedMCTS.search

    def spy_launch(self, *a, **k):
        launches.append((len(a), sorted(k), a[4] if len(a) > 4 else None))
        return real_launch(self, *a, **k)

    def spy_search(self, *a, **k):
        searches.append((len(a), sorted(k)))
        return real_search(self, *a, **k)
    monkeypatch.setattr(engine.BatchedMCTS, "_launch_persistent", spy_launch)
    monkeypatch.setattr(engine.BatchedMCTS, "search", spy_search)
    s = _play(nets, root_noise=None)
    assert s["launches"] == 1 and launches == [(5, ["game", "park"], engine.NO_RULES)] and not searches
    _same(s, plain)
    launches.clear()
    monkeypatch.setenv("IAGO_PERSISTENT_GAMES", "0")
    s = _play(nets, root_noise=None)
    # (a search per turn with today's arguments, each one launch with today's four)
    assert s["launches"] == s["n_turns"] and all(x == (4, ["check", "counts"]) for x in searches)
    assert all(x == (4, [], None) for x in launches) and 1 < len(launches) <= s["n_turns"]
    _same(s, plain)


# ---- 4. the cap of 6 playouts
def test_a_cap_of_6_needs_n_thr_1(nets):
    """At n_thr 15 a fast turn of 6 playouts ends on a fresh root without children: the engine's ValueError, noise or no
    noise.  At n_thr 1 the cap (6, 64) composes: turn 0's fast turns record 5 visits and its full turns 23, and the
    games follow the rules."""
    e = nets[0].SelfPlayEngine(_engine(nets))
    for kw in ({}, dict(root_noise=NOISE)):
        with pytest.raises(ValueError, match="no children"):
            e.play(N_SIMS, playout_cap=(6, 64), **kw)
    e.mcts.close()
    a = _play(nets, engine_kw=dict(n_thr=1), root_noise=NOISE, playout_cap=(6, 64), explore_turns=8, solve_empties=8)
    assert a["launches"] == a["n_turns"]
    kinds = set()
    for g in range(SLOTS):
        full = cap_ref.is_full(SEED, BASE + g, 0, 64)
        kinds.add(full)
        assert a["valid"][0, g] == (1 if full else 4) and int(a["pi"][0, g].sum()) == (N_SIMS if full else 6) - 1, g
        assert a["move"][0, g] == explore_ref.draw(a["pi"][0, g], SEED, BASE + g, 0), g
    assert kinds == {True, False} and (a["valid"] == 3).any()


# ---- 5. guards
def test_guards(nets):
    engine, ops, policy, value, rw = nets
    from iago_amd import _lib
    m = _engine(nets)
    e = engine.SelfPlayEngine(m)
    for bad in ((0, 64), (4097, 64), (77, 257), (77, 64, 100), (77,), 77, (77.0, 64)):
        with pytest.raises(ValueError, match="root_noise"):
            e.play(N_SIMS, root_noise=bad)
        with pytest.raises(ValueError, match="root_noise"):
            e.play_stream(N_SIMS, N_GAMES, root_noise=bad)
    with pytest.raises(TypeError):
        e.play_match(N_SIMS, root_noise=NOISE)
    with pytest.raises(TypeError):
        engine.ArenaEngine.play(None, N_SIMS, root_noise=NOISE)
    # no whole-game launch: the engine's own refusal, and the library's
    m.tree.reset()
    with pytest.raises(ValueError, match="not available with root noise"):
        e._play_persistent(N_SIMS, *e._start_boards(SLOTS), True, engine.PlayRules(None, 0, None, NOISE + (256,)))
    m.close()
    # the persistent engine only
    own = torch.full((8,), engine.START_OWN, dtype=torch.int64, device="cuda")
    opp = torch.full((8,), engine.START_OPP, dtype=torch.int64, device="cuda")
    act = torch.ones(8, dtype=torch.uint8, device="cuda")
    for kw in (dict(use_graph=True), dict(persistent=True, wave=8)):
        m = engine.BatchedMCTS(8, policy, value, rw, n_thr=N_THR, capacity=4096, seed=SEED, game_id_base=BASE, **kw)
        with pytest.raises(ValueError, match="persistent search only"):
            m.search(own, opp, act, N_SIMS, root_noise=NOISE)
        with pytest.raises(ValueError, match="persistent search only"):
            engine.SelfPlayEngine(m, max_turns=4).play(N_SIMS, root_noise=NOISE)
        m.close()
