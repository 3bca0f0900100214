"""Playout-cap randomisation on the GPU (SelfPlayEngine.play / play_stream(playout_cap=(n_fast, full_per_256));
iago_mcts_search_cap, iago_mcts_cap_mask): every searched turn is full (n_sims playouts, valid 1) or fast (the first
n_fast playouts of the same search, valid 4) by the integer rule of tests/playout_cap_ref.py, and everything else is the
plain engine's.  Sizes of test_explore_gpu.py: 64 slots, n_thr 15, capacity 4096, random-init nets, the shipped rollout
weights; 32 playouts, 18 on a fast turn (a fresh root expands at its 16th), a quarter of the turns full."""
import collections
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import mcts_py
from oracle import oracle as orc
from tests import explore_ref, playout_cap_ref as cap
from tests.conftest import load_json

pytestmark = pytest.mark.gpu

SLOTS, N_GAMES, N_SIMS, N_FAST, FULL, BASE, S0, SEED, EXPLORE, N_THR = 64, 160, 32, 18, 64, 300, 1000, 11, 8, 15
CAP = (N_FAST, FULL)
RECORDS = ("own", "opp", "valid", "move", "pi", "z", "final_p1", "final_p2")
VARIANTS = {"cap": {}, "explore": dict(explore_turns=EXPLORE), "solve": dict(solve_empties=8)}


def test_the_inputs_have_both_kinds_of_turn_0():
    full = [cap.is_full(SEED, BASE + g, 0, FULL) for g in range(SLOTS)]
    assert sum(full) >= 4 and SLOTS - sum(full) >= 4


@pytest.fixture(scope="module")
def nets():
    from iago_amd import engine, network, ops
    assert torch.cuda.is_available()
    torch.manual_seed(3)
    policy = network.SLPolicy().cuda().eval()          # random init: broad trees
    value = network.Value().cuda().eval()
    g = load_json("simulate.json")
    return engine, ops, policy, value, ops.RolloutWeights(g["shipped_w"], g["shipped_b"])


def _engine(nets, base=BASE, rw=None, **kw):
    engine, ops, policy, value, shipped = nets
    kw.setdefault("persistent", True)
    m = engine.BatchedMCTS(SLOTS, policy, value, rw or shipped, n_thr=N_THR, capacity=4096, seed=SEED, game_id_base=base, **kw)
    m.sim_counter = S0
    return m


def _host(r):
    out = {k: getattr(r, k).cpu().numpy() for k in RECORDS}
    out["game_turns"] = r.game_turns.cpu().numpy() if r.game_turns is not None else None
    out["n_turns"], out["launches"], out["base"] = r.n_turns, r.launches, r.game_id_base
    out["tuples"] = {k: v.cpu().numpy() for k, v in r.tuples().items()}
    out["fast_tuples"] = {k: v.cpu().numpy() for k, v in r.fast_tuples().items()}
    out["mover"] = list(r.mover)
    return out


def _play(nets, base=BASE, engine_kw=None, max_turns=None, **kw):
    m = _engine(nets, base=base, **(engine_kw or {}))
    if (engine_kw or {}).get("split") and m._split is None:
        m.close()
        pytest.skip("this runtime gives no CU-masked streams")
    e = nets[0].SelfPlayEngine(m) if max_turns is None else nets[0].SelfPlayEngine(m, max_turns=max_turns)
    out = _host(e.play(N_SIMS, **kw))
    out["sim"], out["split"], out["evals"] = m.sim_counter, m._split is not None, m.n_leaf_evals
    m.close()
    return out


@pytest.fixture(scope="module")
def plain(nets):
    return _play(nets)


@pytest.fixture(scope="module")
def capped(nets):
    return {k: _play(nets, playout_cap=CAP, **kw) for k, kw in VARIANTS.items()}


def _same(a, b, keys=RECORDS + ("n_turns", "sim")):
    for k in keys:
        assert np.array_equal(a[k], b[k]), k


def _searched_rows(s):
    T, B = s["valid"].shape
    return [(t, g) for g in range(B) for t in range(T) if s["valid"][t, g] in (1, 4)]


# ---- 1. the valid codes of one launch against the reference
def test_one_launch_records_full_and_fast_turns_by_the_reference(capped):
    s = capped["cap"]
    assert s["launches"] == 1
    rows = _searched_rows(s)
    for t, g in rows:
        assert s["valid"][t, g] == cap.valid_code(SEED, s["base"] + g, t, FULL), (g, t)
    codes = {int(s["valid"][t, g]) for t, g in rows}
    assert codes == {1, 4}
    assert set(np.unique(s["valid"]).tolist()) <= {0, 1, 4}
    # (a fresh root expands at its 16th playout: turn 0's children hold the budget's other playouts)
    for g in range(SLOTS):
        assert int(s["pi"][0, g].sum()) == cap.budget(SEED, BASE + g, 0, FULL, N_SIMS, N_FAST) - N_THR, g
    n_full, n_fast = int((s["valid"] == 1).sum()), int((s["valid"] == 4).sum())
    assert s["evals"] == n_full * N_SIMS + n_fast * N_FAST


# ---- 2. the oracle replay of one launch
def _check_rules(s, explore_turns=0, solved_from=None):
    """test_explore_gpu._check_rules with a searched row being valid 1 or 4, as the reference says, its visit row at
    least the turn's budget less the n_thr playouts a fresh root spends on itself."""
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
                        assert s["valid"][t, G] == cap.valid_code(SEED, s["base"] + G, t, FULL), (G, t)
                        assert np.all(row[[x for x in range(64) if x not in acts]] == 0), (G, t)
                        n = cap.budget(SEED, s["base"] + G, t, FULL, N_SIMS, N_FAST)
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
def test_one_launch_follows_the_rules(capped, variant):
    s = capped[variant]
    assert s["launches"] == (2 if variant == "solve" else 1)
    _check_rules(s, explore_turns=EXPLORE if variant == "explore" else 0, solved_from=8 if variant == "solve" else None)


# ---- 3. the budget, independently: the oracle's search after N_SIMS / N_FAST playouts
def test_turn_0_is_the_oracles_search_after_the_budget(nets):
    """Four full and four fast games of turn 0: the recorded visit row is the root of oracle/mcts_py.MCTS after N_SIMS /
    N_FAST playouts, fed the same nets and the rollouts of the same Philox streams (stream sim_counter + playout) -- as
    tests/test_match_gpu.py feeds PV-MCTS's first searches, uniform rollout weights included (the oracle plays them)."""
    from tests.test_mcts_production_gpu import NetProbe
    engine, ops, policy, value, _ = nets
    s = _play(nets, engine_kw=dict(rw=ops.uniform_weights()), max_turns=2, playout_cap=CAP)
    probe = NetProbe(ops, policy, value)
    full = [g for g in range(SLOTS) if cap.is_full(SEED, BASE + g, 0, FULL)][:4]
    fast = [g for g in range(SLOTS) if not cap.is_full(SEED, BASE + g, 0, FULL)][:4]
    assert len(full) == 4 and len(fast) == 4
    for g in full + fast:
        n = N_SIMS if g in full else N_FAST
        counter = [S0]

        def roll(state, color, g=g, counter=counter):
            z = orc.random_playout(state, color, seed=SEED, game_id=BASE + g, stream=counter[0])[0]
            counter[0] += 1
            return z

        om = mcts_py.MCTS(probe.policy_fn, probe.value_fn, roll, lmbda=0.5, c_puct=1.0, n_thr=N_THR)
        got = om.get_move(np.array(orc.initial_state(), dtype=np.float32), 1, n)
        want = np.zeros(64, np.int64)
        for b, ch in om.root.children.items():
            if b >= 0:
                want[b] = ch.n_visits
        assert np.array_equal(want, s["pi"][0, g]), (g, n)
        assert int(want.sum()) == n - N_THR and got == int(s["move"][0, g]), g
        assert s["valid"][0, g] == (1 if g in full else 4), g


# ---- 4. the same games record for record
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_turn_loop_plays_the_same_games(nets, capped, variant, monkeypatch):
    monkeypatch.setenv("IAGO_PERSISTENT_GAMES", "0")
    s = _play(nets, playout_cap=CAP, **VARIANTS[variant])
    assert s["launches"] == s["n_turns"] > 1
    _same(s, capped[variant])
    assert s["evals"] == capped[variant]["evals"]


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_role_split_plays_the_same_games(nets, capped, variant):
    s = _play(nets, engine_kw=dict(split=8), playout_cap=CAP, **VARIANTS[variant])   # (skips without CU-masked streams)
    assert s["split"] and s["launches"] == capped[variant]["launches"]
    _same(s, capped[variant])


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_stream_equals_the_batch_loop(nets, capped, variant):
    kw = VARIANTS[variant]
    parts = [capped[variant]] + [_play(nets, base=BASE + k * SLOTS, playout_cap=CAP, **kw) for k in (1, 2)]
    m = _engine(nets)
    s = _host(nets[0].SelfPlayEngine(m).play_stream(N_SIMS, N_GAMES, playout_cap=CAP, **kw))
    sim, ctl3 = m.sim_counter, int(m._ps["ctl"][3].item())
    m.close()
    assert s["launches"] == (2 if variant == "solve" else 1) and ctl3 == 0 and s["valid"].shape[1] == N_GAMES
    for G in range(N_GAMES):
        b, c = parts[G // SLOTS], G % SLOTS
        t = int(b["game_turns"][c])
        assert int(s["game_turns"][G]) == t, G
        for k in ("z", "final_p1", "final_p2"):
            assert s[k][G] == b[k][c], (G, k)
        for k in ("own", "opp", "valid", "move", "pi"):
            assert np.array_equal(s[k][:t, G], b[k][:t, c]), (G, k)
    assert s["n_turns"] == int(s["game_turns"].max())
    assert sim == (S0 + s["n_turns"] * N_SIMS) & 0xFFFFFFFF
    for t, G in _searched_rows(s):                       # (the game's own id, whichever slot played it)
        assert s["valid"][t, G] == cap.valid_code(SEED, BASE + G, t, FULL), (G, t)
    assert (s["valid"] == 4).sum() > (s["valid"] == 1).sum() > 0


# ---- 5. degenerate settings
def test_every_turn_full_is_the_plain_engine(nets, plain):
    s = _play(nets, playout_cap=(N_FAST, 256))
    assert s["launches"] == 1
    _same(s, plain)
    assert s["evals"] == plain["evals"] and len(s["fast_tuples"]["z"]) == 0


def test_a_fast_turn_of_n_sims_playouts_changes_the_code_only(nets, plain):
    s = _play(nets, playout_cap=(N_SIMS, FULL))
    _same(s, plain, keys=tuple(k for k in RECORDS if k != "valid") + ("n_turns", "sim"))
    assert np.array_equal(s["valid"] != 0, plain["valid"] != 0)
    for t, g in _searched_rows(s):
        assert plain["valid"][t, g] == 1 and s["valid"][t, g] == cap.valid_code(SEED, BASE + g, t, FULL), (g, t)
    assert (s["valid"] == 4).any() and (s["valid"] == 1).any()
    assert s["evals"] == plain["evals"]


# ---- 6. tuples and refusals
def test_tuples_are_the_full_rows_and_fast_tuples_the_fast_ones(capped):
    s = capped["cap"]
    for name, code in (("tuples", 1), ("fast_tuples", 4)):
        tp = s[name]
        t, g = tp["turn"], tp["game"] - BASE
        assert len(t) == int((s["valid"] == code).sum()) > 0
        assert np.all(s["valid"][t, g] == code)
        assert len(set(zip(t.tolist(), g.tolist()))) == len(t)
        assert np.array_equal(tp["pi"], s["pi"][t, g]) and np.array_equal(tp["move"], s["move"][t, g])
        assert np.array_equal(tp["own"], s["own"][t, g]) and np.array_equal(tp["opp"], s["opp"][t, g])
        sign = np.array([1 if c == 1 else -1 for c in s["mover"]])
        assert np.array_equal(tp["z"], s["z"][g].astype(np.int64) * sign[t])   # z from the mover's view
        assert np.array_equal(tp["colour"], np.array(s["mover"])[t])


def test_none_is_todays_play(nets, plain, monkeypatch):
    """playout_cap = None launches what the plain engine launches: iago_mcts_search_persistent, or iago_mcts_search_split
    where the engine set the role split up -- once for whole games in one launch, once per searched turn in the turn
    loop -- and never the hand-over's, the draw's or the cap's entry point."""
    from iago_amd import _lib, ops

    def never(*a, **k):
        raise AssertionError("playout_cap = None reached the playout cap's entry points")
    monkeypatch.setattr(ops, "search_cap", never)
    monkeypatch.setattr(ops, "playout_cap_mask", never)
    lib, calls = _lib.lib(), collections.Counter()
    for name in ("persistent", "split", "park", "explore", "cap"):
        def counted(*a, _f=getattr(lib, "iago_mcts_search_" + name), _name=name):
            calls[_name] += 1
            return _f(*a)
        monkeypatch.setattr(lib, "iago_mcts_search_" + name, counted)
    s = _play(nets, playout_cap=None)
    entry = "split" if s["split"] else "persistent"
    assert s["launches"] == 1 and dict(calls) == {entry: 1}
    _same(s, plain)
    calls.clear()
    monkeypatch.setenv("IAGO_PERSISTENT_GAMES", "0")
    s = _play(nets, playout_cap=None)
    # (a launch per turn that somebody searches, each through the plain engine's entry point)
    assert s["launches"] == s["n_turns"] and set(calls) == {entry} and 1 < calls[entry] <= s["n_turns"]
    _same(s, plain)


def test_guards(nets):
    engine, ops = nets[0], nets[1]
    from iago_amd import _lib
    m = _engine(nets)
    e = engine.SelfPlayEngine(m)
    for bad in ((0, FULL), (N_SIMS + 1, FULL), (N_FAST, 0), (N_FAST, 257), (N_FAST,), N_FAST, (1.0, FULL)):
        with pytest.raises(ValueError, match="playout_cap"):
            e.play(N_SIMS, playout_cap=bad)
        with pytest.raises(ValueError, match="playout_cap"):
            e.play_stream(N_SIMS, N_GAMES, playout_cap=bad)
    with pytest.raises(TypeError):
        e.play_match(N_SIMS, playout_cap=CAP)
    with pytest.raises(TypeError):
        engine.ArenaEngine.play(None, N_SIMS, playout_cap=CAP)
    # the library's own refusals, with the entry point named: the launch of whole games with each bad argument
    dev = m.cur_own.device
    own, opp = e._start_boards(SLOTS)
    rec = e._new_records(SLOTS)
    g = dict(max_turns=e.max_turns, games_total=0, own=own, opp=opp, n_turns=torch.zeros(SLOTS, dtype=torch.int32, device=dev),
             **{"rec_" + k: v for k, v in rec.items()})
    active = torch.ones(SLOTS, dtype=torch.uint8, device=dev)
    lib = _lib.lib()

    def refused(a, what, n_fast=N_FAST, full=FULL, explore=0, reserved0=0, reserved=0, park=None):
        c = _lib.SearchCapArgs()
        c.n_fast, c.full_per_256, c.explore_turns, c.reserved0 = n_fast, full, explore, reserved0
        c.reserved[2] = reserved
        c.park = C.addressof(park) if park is not None else None
        assert lib.iago_mcts_search_cap(C.byref(a), C.byref(c), None) == _lib.IAGO_ERR_INVALID, what
        err = lib.iago_last_error()
        assert err.startswith(b"iago_mcts_search_cap") and what in err, err

    m.tree.reset()
    a, keep = m._search_args(None, None, active, N_SIMS, g)
    assert lib.iago_mcts_search_cap(None, None, None) == _lib.IAGO_ERR_INVALID
    assert lib.iago_mcts_search_cap(C.byref(a), None, None) == _lib.IAGO_ERR_INVALID
    refused(a, b"n_fast", n_fast=0)
    refused(a, b"n_fast", n_fast=N_SIMS + 1)
    refused(a, b"full_per_256", full=0)
    refused(a, b"full_per_256", full=257)
    refused(a, b"reserved", reserved0=1)
    refused(a, b"reserved", reserved=1)
    refused(a, b"explore_turns", explore=-1)
    refused(a, b"explore_turns", explore=129)
    refused(a, b"park", park=_lib.SearchParkArgs())
    codes = active.clone()
    codes[5] = _lib.MATCH_MCTS_COLOUR_2
    a2, keep2 = m._search_args(None, None, codes, N_SIMS, g)
    refused(a2, b"match codes")
    a3, keep3 = m._search_args(own, opp, active, N_SIMS)          # (one search: max_turns == 0)
    refused(a3, b"whole games")
    with pytest.raises(_lib.IagoError, match=r"\(-1\)"):
        e._play_persistent(N_SIMS, own, opp, True, engine.PlayRules(None, 0, CAP), active=codes)
    assert int(m._ps["ctl"][3].item()) == 0
    m.close()


def test_per_playout_engine_caps_through_the_turn_loop(nets):
    """use_graph=True (no persistent search): the argument is honoured by the turn loop's two searches per turn."""
    engine, ops, policy, value, rw = nets
    m = engine.BatchedMCTS(8, policy, value, rw, n_thr=N_THR, capacity=4096, seed=SEED, game_id_base=BASE, use_graph=True)
    assert not getattr(m, "persistent", False)
    r = engine.SelfPlayEngine(m, max_turns=6).play(N_SIMS, playout_cap=CAP)
    valid, pi = r.valid.cpu().numpy(), r.pi.cpu().numpy()
    assert r.launches == r.n_turns == 6
    for g in range(8):
        for t in range(6):
            assert valid[t, g] == cap.valid_code(SEED, BASE + g, t, FULL), (g, t)
        assert int(pi[0, g].sum()) == cap.budget(SEED, BASE + g, 0, FULL, N_SIMS, N_FAST) - N_THR, g
    m.close()
