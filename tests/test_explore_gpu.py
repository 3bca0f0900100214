"""Exploring self-play on the GPU (SelfPlayEngine.play / play_stream(explore_turns=); iago_mcts_search_explore,
iago_mcts_draw_move): at the searched turns t < explore_turns the move is drawn from the root's visit counts by the
integer rule of tests/explore_ref.py -- the records carry everything the reference needs (the visit row, the game's id,
the turn) -- and everything else is the plain engine's, bit for bit.  Sizes of test_selfplay_stream_gpu.py: 64 slots, 24
playouts, n_thr 15, random-init nets, the shipped rollout weights."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import explore_ref
from tests.conftest import load_json

pytestmark = pytest.mark.gpu

SLOTS, N_GAMES, N_SIMS, BASE, S0, SEED, EXPLORE = 64, 160, 24, 300, 1000, 11, 8
RECORDS = ("own", "opp", "valid", "move", "pi", "z", "final_p1", "final_p2")


@pytest.fixture(scope="module")
def nets():
    from iago_amd import engine, network, ops
    assert torch.cuda.is_available()
    torch.manual_seed(3)
    policy = network.SLPolicy().cuda().eval()          # random init: broad trees
    value = network.Value().cuda().eval()
    g = load_json("simulate.json")
    return engine, ops, policy, value, ops.RolloutWeights(g["shipped_w"], g["shipped_b"])


def _engine(nets, base=BASE, **kw):
    engine, ops, policy, value, rw = nets
    kw.setdefault("persistent", True)
    m = engine.BatchedMCTS(SLOTS, policy, value, rw, n_thr=15, capacity=4096, seed=SEED, game_id_base=base, **kw)
    m.sim_counter = S0
    return m


def _host(r):
    out = {k: getattr(r, k).cpu().numpy() for k in RECORDS}
    out["game_turns"] = r.game_turns.cpu().numpy() if r.game_turns is not None else None
    out["n_turns"], out["launches"], out["base"] = r.n_turns, r.launches, r.game_id_base
    return out


def _play(nets, base=BASE, engine_kw=None, **kw):
    m = _engine(nets, base=base, **(engine_kw or {}))
    out = _host(nets[0].SelfPlayEngine(m).play(N_SIMS, **kw))
    out["sim"] = m.sim_counter
    m.close()
    return out


@pytest.fixture(scope="module")
def plain(nets):
    return _play(nets)


@pytest.fixture(scope="module")
def explored(nets):
    return _play(nets, explore_turns=EXPLORE)


def _check_moves(s, explore_turns, cols=None, rows=None):
    """Every searched row: below explore_turns the reference's draw from the row's own visit counts, from there on
    the first maximum.  Returns (rows drawn, rows where the draw is not the first maximum)."""
    drawn = differ = 0
    T, B = s["valid"].shape
    for g in range(B) if cols is None else cols:
        for t in range(T if rows is None else rows):
            if s["valid"][t, g] != 1:
                continue
            row, a = s["pi"][t, g], int(s["move"][t, g])
            if t < explore_turns:
                want = explore_ref.draw(row, SEED, s["base"] + g, t)
                assert a == want, (g, t, a, want, row[row > 0])
                drawn += 1
                differ += a != int(np.argmax(row))
            else:
                assert a == int(np.argmax(row)), (g, t)
    return drawn, differ


def _check_rules(s, explore_turns, solved_from=None):
    """The oracle replay of test_selfplay_stream_gpu.py over the records of s (no handicap), the searched move being
    the reference's draw below explore_turns: the recorded position, search or pass by the mover's legal set, a legal
    move on visited cells only, the books ending the game at its recorded turn, the result and the final board."""
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
                        assert s["valid"][t, G] == 1, (G, t)
                        assert np.all(row[[x for x in range(64) if x not in acts]] == 0), (G, t)
                        assert row[a] > 0 and int(row.sum()) >= N_SIMS - 15, (G, t)
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


def _same(a, b, keys=RECORDS + ("n_turns", "sim")):
    for k in keys:
        assert np.array_equal(a[k], b[k]), k


# ---- 1. the one launch against the reference
def test_one_launch_draws_by_the_reference(explored):
    s = explored
    assert s["launches"] == 1
    drawn, differ = _check_moves(s, EXPLORE)
    assert drawn == SLOTS * EXPLORE          # (no pass in the first 8 turns from the opening)
    assert differ > 0                        # the draw is not the argmax in disguise
    _check_rules(s, EXPLORE)


# ---- 2. one launch == turn loop
def test_turn_loop_plays_the_same_games(nets, explored, monkeypatch):
    monkeypatch.setenv("IAGO_PERSISTENT_GAMES", "0")
    s = _play(nets, explore_turns=EXPLORE)
    assert s["launches"] == s["n_turns"] > 1
    _same(s, explored)


# ---- 3. the stream and the role split == the batch loop
@pytest.fixture(scope="module")
def batches(nets, explored):
    return [explored] + [_play(nets, base=BASE + k * SLOTS, explore_turns=EXPLORE) for k in (1, 2)]


def _stream(nets, **engine_kw):
    m = _engine(nets, **engine_kw)
    r = nets[0].SelfPlayEngine(m).play_stream(N_SIMS, N_GAMES, explore_turns=EXPLORE)
    out = _host(r)
    out["sim"], out["split"], out["ctl3"] = m.sim_counter, m._split is not None, int(m._ps["ctl"][3].item())
    m.close()
    return out


def _assert_equals_batches(s, parts):
    assert s["launches"] == 1 and s["ctl3"] == 0 and s["valid"].shape[1] == N_GAMES
    for G in range(N_GAMES):
        b, c = parts[G // SLOTS], G % SLOTS
        t = int(b["game_turns"][c])
        assert int(s["game_turns"][G]) == t, G
        for k in ("z", "final_p1", "final_p2"):
            assert s[k][G] == b[k][c], (G, k)
        for k in ("own", "opp", "valid", "move", "pi"):
            assert np.array_equal(s[k][:t, G], b[k][:t, c]), (G, k)
    assert s["n_turns"] == int(s["game_turns"].max())
    assert s["sim"] == (S0 + s["n_turns"] * N_SIMS) & 0xFFFFFFFF


def test_stream_equals_the_batch_loop(nets, batches):
    s = _stream(nets)
    _assert_equals_batches(s, batches)
    drawn, differ = _check_moves(s, EXPLORE, rows=EXPLORE)       # (the game's own id, whichever slot played it)
    assert drawn == N_GAMES * EXPLORE and differ > 0


def test_role_split_plays_the_same_stream(nets, batches):
    s = _stream(nets, split=8)
    if not s["split"]:
        pytest.skip("this runtime gives no CU-masked streams")
    _assert_equals_batches(s, batches)


# ---- 4. off is off
@pytest.mark.parametrize("off", [None, 0])
def test_none_and_zero_are_todays_play(nets, plain, off, monkeypatch):
    from iago_amd import ops

    def never(*a, **k):
        raise AssertionError("explore_turns = %r reached iago_mcts_search_explore" % (off,))
    monkeypatch.setattr(ops, "search_explore", never)
    monkeypatch.setattr(ops, "draw_move", never)
    s = _play(nets, explore_turns=off)
    assert s["launches"] == 1
    _same(s, plain)
    _check_moves(s, 0)


# ---- 5. with the endgame solver
def test_explore_composes_with_solve_empties(nets, explored):
    s = _play(nets, explore_turns=EXPLORE, solve_empties=8)
    assert s["launches"] == 2
    drawn, _ = _check_moves(s, EXPLORE)
    assert drawn == SLOTS * EXPLORE
    _check_rules(s, EXPLORE, solved_from=8)
    solved = 0
    for g in range(SLOTS):
        v = s["valid"][:, g]
        # (a game that ended by two passes above 8 empties has nothing to solve: the unsolved game, whole)
        first = int(np.argmax(v == 3)) if (v == 3).any() else int(s["game_turns"][g])
        solved += int((v == 3).any())
        assert not (v[first:] == 1).any(), g            # the solved tail: the solver's moves and passes only
        # the rows before the hand-over are the unsolved game's
        for k in ("own", "opp", "valid", "move", "pi"):
            assert np.array_equal(s[k][:first, g], explored[k][:first, g]), (g, k)
    assert solved > SLOTS // 2


# ---- 6. the standalone draw
def test_draw_move_equals_the_reference_on_best_moves_rows(nets):
    engine, ops = nets[0], nets[1]
    m = _engine(nets)
    own = torch.full((SLOTS,), engine.START_OWN, dtype=torch.int64, device="cuda")
    opp = torch.full((SLOTS,), engine.START_OPP, dtype=torch.int64, device="cuda")
    act = torch.ones(SLOTS, dtype=torch.uint8, device="cuda")
    m.tree.reset()
    m.search(own, opp, act, N_SIMS)
    mv, vis = m.best_move(act)
    best, rows = mv.cpu().numpy().copy(), vis.cpu().numpy().copy()
    assert (rows.sum(axis=1) > 0).all()
    differ = 0
    for t in range(EXPLORE):
        mv, vis = m.draw_move(t, act)
        got, got_rows = mv.cpu().numpy(), vis.cpu().numpy()
        assert np.array_equal(got_rows, rows), t
        want = [explore_ref.draw(rows[g], SEED, BASE + g, t) for g in range(SLOTS)]
        assert got.tolist() == want, t
        differ += int((got != best).sum())
    assert differ > 0
    # the raw op: per-game ids and turns, an inactive game untouched, no visit row asked for
    ids = torch.arange(SLOTS, dtype=torch.int32, device="cuda").flip(0) + 7
    turns = (torch.arange(SLOTS, dtype=torch.int32, device="cuda") * 5) % 13
    out = torch.full((SLOTS,), 99, dtype=torch.int8, device="cuda")
    act[3] = 0
    ops.draw_move(m.tree.ref(), act, SEED, ids, turns, out)
    got = out.cpu().numpy()
    for g in range(SLOTS):
        want = 99 if g == 3 else explore_ref.draw(rows[g], SEED, int(ids[g]), int(turns[g]))
        assert got[g] == want, g
    m.close()


# ---- 7. diversity, as a condition
def _prefixes(s):
    return {tuple(s["move"][:EXPLORE, g].tolist()) for g in range(s["move"].shape[1])}


def test_exploring_games_leave_the_opening_on_more_lines(nets, plain, explored):
    """Among 64 games, strictly more distinct 8-turn move prefixes with explore_turns = 8 than without.  At the
    engine's default lmbda = 0.5 the condition cannot be met by anything: with random-init nets the rollouts' Philox
    streams alone already put the 64 games on 64 different lines (measured: 64 plain, 64 explored -- printed below),
    and 64 is the most there is.  The batch that collapses is the one the draw is for -- no rollout in the leaf value
    (lmbda = 0), where nothing but the game's id distinguishes one game from another: there the plain games are one
    line, and the condition is asked of that batch, at the same sizes."""
    print("lmbda 0.5: distinct 8-turn openings among 64 games: %d plain, %d explored"
          % (len(_prefixes(plain)), len(_prefixes(explored))))
    a = len(_prefixes(_play(nets, engine_kw=dict(lmbda=0.0))))
    b = len(_prefixes(_play(nets, engine_kw=dict(lmbda=0.0), explore_turns=EXPLORE)))
    print("lmbda 0: distinct 8-turn openings among 64 games: %d plain, %d explored" % (a, b))
    assert a == 1          # (the same search 64 times)
    assert b > a


# ---- 8. guards
def test_guards(nets):
    engine, ops = nets[0], nets[1]
    from iago_amd import _lib
    m = _engine(nets)
    e = engine.SelfPlayEngine(m)
    with pytest.raises(ValueError, match="explore_turns"):
        e.play(N_SIMS, explore_turns=-1)
    with pytest.raises(ValueError, match="explore_turns"):
        e.play_stream(N_SIMS, N_GAMES, explore_turns=-1)
    with pytest.raises(TypeError):
        e.play_match(N_SIMS, explore_turns=EXPLORE)
    # match codes in the launch are refused on the host, with the entry point named
    codes = torch.ones(SLOTS, dtype=torch.uint8, device="cuda")
    codes[5] = _lib.MATCH_MCTS_COLOUR_2
    m.tree.reset()
    with pytest.raises(_lib.IagoError, match=r"\(-1\)"):
        e._play_persistent(N_SIMS, *e._start_boards(SLOTS), True, engine.PlayRules(None, EXPLORE, None), active=codes)
    err = _lib.lib().iago_last_error()
    assert err.startswith(b"iago_mcts_search_explore") and b"match codes" in err
    m.close()


def test_per_playout_engine_explores_through_the_turn_loop(nets):
    """use_graph=True (no persistent search): the argument is honoured by the turn loop's draw_move."""
    engine, ops, policy, value, rw = nets
    m = engine.BatchedMCTS(8, policy, value, rw, n_thr=15, capacity=4096, seed=SEED, game_id_base=BASE, use_graph=True)
    assert not getattr(m, "persistent", False)
    r = engine.SelfPlayEngine(m, max_turns=12).play(N_SIMS, explore_turns=EXPLORE)
    s = {k: getattr(r, k).cpu().numpy() for k in ("valid", "move", "pi")}
    s["base"] = r.game_id_base
    assert r.launches == r.n_turns == 12
    drawn, differ = _check_moves(s, EXPLORE)
    assert drawn == 8 * EXPLORE
    m.close()
