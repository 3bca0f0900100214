"""The self-play stream (SelfPlayEngine.play_stream; iago_mcts_search_args.games_total): n_games whole games through the
engine's B slots in ONE persistent launch -- a slot whose game ends claims the next game id on the device, resets its
tree and plays that game.  What must hold: game G of the stream is bit for bit game G of the BATCH LOOP (play()
ceil(n_games / B) times, batch k with game_id_base + k B, every batch from the same sim_counter), whichever slot played
it and whenever -- records, visit counts, moves, results, final boards, turns -- under any schedule and in the role
split; and every record obeys the rules (the C oracle)."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests.conftest import load_json

pytestmark = pytest.mark.gpu

SLOTS, N_GAMES, N_SIMS, BASE, S0 = 64, 160, 24, 300, 1000
HANDICAP = 2 * 8 + 4        # the extra colour-2 stone of src/train_rl.py:43-46, on the odd games


@pytest.fixture(scope="module")
def nets():
    from iago_amd import engine, network, ops
    assert torch.cuda.is_available()
    torch.manual_seed(3)
    policy = network.SLPolicy().cuda().eval()          # random init: broad trees
    value = network.Value().cuda().eval()
    g = load_json("simulate.json")
    return engine, ops, policy, value, ops.RolloutWeights(g["shipped_w"], g["shipped_b"])


def _engine(nets, **kw):
    engine, ops, policy, value, rw = nets
    m = engine.BatchedMCTS(SLOTS, policy, value, rw, n_thr=15, capacity=4096, seed=11, game_id_base=BASE,
                           persistent=True, **kw)
    m.sim_counter = S0
    return m


def _handicap(n):
    hc = torch.zeros(n, dtype=torch.int64, device="cuda")
    hc[1::2] = 1 << HANDICAP
    return hc


def _host(r):
    out = {k: getattr(r, k).cpu().numpy() for k in ("own", "opp", "valid", "move", "pi", "z", "final_p1", "final_p2",
                                                      "game_turns")}
    out["n_turns"] = r.n_turns
    return out


def _tuples(r):
    t = r.tuples()
    t = {k: v.cpu().numpy() for k, v in t.items()}
    order = np.lexsort((t["turn"], t["game"]))
    return {k: v[order] for k, v in t.items()}


@pytest.fixture(scope="module")
def batch_loop(nets):
    """The games of the stream, played as the batch loop from play() (built here, not by the engine)."""
    engine = nets[0]
    m = _engine(nets)
    hc = _handicap(3 * SLOTS)
    parts = []
    for k in range(3):                       # 160 games = 2.5 batches of 64: the last one partial
        m.game_id_base, m.sim_counter = BASE + k * SLOTS, S0
        r = engine.SelfPlayEngine(m).play(N_SIMS, handicap=hc[k * SLOTS:(k + 1) * SLOTS])
        assert r.game_turns is not None and r.game_id_base == BASE + k * SLOTS
        parts.append((_host(r), _tuples(r)))
    m.close()
    tup = {k: np.concatenate([t[k] for _, t in parts]) for k in parts[0][1]}
    keep = tup["game"] < BASE + N_GAMES
    tup = {k: v[keep] for k, v in tup.items()}
    return parts, tup


def _stream(nets, n_games=N_GAMES, **kw):
    engine = nets[0]
    m = _engine(nets, **kw)
    r = engine.SelfPlayEngine(m).play_stream(N_SIMS, n_games, handicap=_handicap(n_games))
    out = _host(r)
    out["launches"], out["sim"], out["split"] = r.launches, m.sim_counter, m._split is not None
    out["tuples"] = _tuples(r)
    out["ctl3"] = int(m._ps["ctl"][3].item())
    m.close()
    return out


@pytest.fixture(scope="module")
def stream(nets):
    return _stream(nets)


def _assert_equals_batches(s, parts, n_games):
    """Game G of the stream = column G % 64 of batch G // 64, on the rows the game played."""
    for G in range(n_games):
        b, c = parts[G // SLOTS][0], G % SLOTS
        t = int(b["game_turns"][c])
        assert int(s["game_turns"][G]) == t, G
        for k in ("z", "final_p1", "final_p2"):
            assert s[k][G] == b[k][c], (G, k)
        for k in ("own", "opp", "valid", "move", "pi"):
            assert np.array_equal(s[k][:t, G], b[k][:t, c]), (G, k)
    assert s["n_turns"] == int(s["game_turns"].max())


def test_stream_equals_the_batch_loop(stream, batch_loop):
    parts, tup = batch_loop
    s = stream
    assert s["launches"] == 1 and s["ctl3"] == 0            # ONE launch, not given up
    assert s["valid"].shape[1] == N_GAMES and len(s["z"]) == N_GAMES
    _assert_equals_batches(s, parts, N_GAMES)
    # the training tuples: global ids BASE .. BASE + 159, row for row
    assert set(np.unique(s["tuples"]["game"])) == set(range(BASE, BASE + N_GAMES))
    for k in tup:
        assert np.array_equal(s["tuples"][k], tup[k]), k
    assert s["sim"] == (S0 + s["n_turns"] * N_SIMS) & 0xFFFFFFFF
    assert s["valid"].sum() > N_GAMES * 50


@pytest.mark.parametrize("env,net", [(dict(IAGO_PERSISTENT_GPW="16", IAGO_PERSISTENT_PACE="1",
                                           IAGO_PERSISTENT_PACE_BACKLOG="0"), 6),
                                     (dict(IAGO_PERSISTENT_GPW="8", IAGO_PERSISTENT_PACE="-1"), None)])
def test_scheduling_does_not_change_the_games(nets, stream, env, net, monkeypatch):
    """Games per game workgroup, few net workgroups, the pacing at its most intrusive (a game one playout ahead of the
    mean holds whenever anything waits) or off: WHEN a slot takes which game changes, the games do not."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s = _stream(nets, net_workgroups=net)
    assert s["launches"] == 1
    for k in ("own", "opp", "valid", "move", "pi", "z", "final_p1", "final_p2", "game_turns", "n_turns", "sim"):
        assert np.array_equal(s[k], stream[k]), k


def test_role_split_plays_the_same_stream(nets, stream):
    s = _stream(nets, split=8)
    if not s["split"]:
        pytest.skip("this runtime gives no CU-masked streams")
    assert s["launches"] == 1 and s["ctl3"] == 0
    for k in ("own", "opp", "valid", "move", "pi", "z", "final_p1", "final_p2", "game_turns", "n_turns", "sim"):
        assert np.array_equal(s[k], stream[k]), k


def test_stream_records_follow_the_rules(stream):
    """Every record of every game of the stream through the C oracle (oracle/othello_oracle.c): the recorded position,
    search or pass by the mover's legal set, a legal and most visited move, the books of game.py:117-142,253-255
    ending the game at its recorded turn, the result (rl_env.py:141-149) and the final board."""
    s = dict(stream)
    for k in ("own", "opp", "final_p1", "final_p2"):
        s[k] = s[k].view(np.uint64)                         # (bit 63 set: a negative int64)
    n_rec = 0
    for G in range(N_GAMES):
        state = orc.initial_state(handicap=divmod(HANDICAP, 8) if G % 2 else None)
        stone_num, pass_flg, t, over = 4, False, 0, False
        while not over and t < 128:
            for color in (1, 2):
                p1, p2 = orc.state_to_bits(state)
                mover = (p1, p2) if color == 1 else (p2, p1)
                assert (int(s["own"][t, G]), int(s["opp"][t, G])) == mover, (G, t)
                acts = orc.legal_actions(state, color)
                row = s["pi"][t, G]
                if len(acts) > 0:
                    a = int(s["move"][t, G])
                    assert s["valid"][t, G] == 1 and a in acts, (G, t, a)
                    assert np.all(row[[x for x in range(64) if x not in acts]] == 0), (G, t)
                    assert a == int(np.argmax(row)) and int(row.sum()) >= N_SIMS - 15, (G, t)
                    orc.place_stone(state, a, color)
                    stone_num += 1
                    pass_flg = False
                else:
                    assert s["valid"][t, G] == 0 and s["move"][t, G] == -1 and not row.any(), (G, t)
                    if pass_flg:
                        stone_num = 64
                    pass_flg = True
                n_rec += 1
                t += 1
            if stone_num >= 64:
                over = True
        assert over and t % 2 == 0 and int(s["game_turns"][G]) == t, (G, t)
        assert s["z"][G] == orc.judge(state, 1), G
        assert orc.state_to_bits(state) == (int(s["final_p1"][G]), int(s["final_p2"][G])), G
    assert n_rec == int(s["game_turns"].sum())


def test_the_abi_refuses_bad_stream_arguments(nets):
    """games_total > 0 needs whole games (max_turns > 0) and no slot-indexed diagnostics (z_log); games_total < 0 is
    refused: IAGO_ERR_INVALID, with the entry point named in iago_last_error()."""
    from iago_amd import _lib
    engine = nets[0]
    T, n = 128, 96
    for z_rows, max_turns, games_total in ((0, 0, n), (0, T, -1), (64, T, n)):
        m = engine.BatchedMCTS(SLOTS, *nets[2:], n_thr=15, capacity=1024, seed=1, persistent=True, split=0,
                               z_log_rows=z_rows)
        dev = "cuda"
        g = dict(max_turns=max_turns, games_total=games_total,
                 own=torch.full((n,), engine.START_OWN, dtype=torch.int64, device=dev),
                 opp=torch.full((n,), engine.START_OPP, dtype=torch.int64, device=dev),
                 n_turns=torch.zeros(n, dtype=torch.int32, device=dev),
                 rec_own=torch.zeros((T, n), dtype=torch.int64, device=dev),
                 rec_opp=torch.zeros((T, n), dtype=torch.int64, device=dev),
                 rec_valid=torch.zeros((T, n), dtype=torch.uint8, device=dev),
                 rec_move=torch.zeros((T, n), dtype=torch.int8, device=dev),
                 rec_pi=torch.zeros((T, n, 64), dtype=torch.int32, device=dev))
        active = torch.ones(SLOTS, dtype=torch.uint8, device=dev)
        own = torch.full((SLOTS,), engine.START_OWN, dtype=torch.int64, device=dev)
        opp = torch.full((SLOTS,), engine.START_OPP, dtype=torch.int64, device=dev)
        with pytest.raises(_lib.IagoError, match=r"\(-1\)"):         # IAGO_ERR_INVALID
            m._launch_persistent(own, opp, active, N_SIMS, game=g)
        assert b"iago_mcts_search_persistent" in _lib.lib().iago_last_error()
        assert b"games_total" in _lib.lib().iago_last_error()
        m.close()


def test_fewer_games_than_slots(nets, batch_loop):
    """n_games <= B: the first n_games games of one play() batch; the other slots play nothing."""
    parts = batch_loop[0]
    s = _stream(nets, n_games=40)
    assert s["launches"] == 1 and s["valid"].shape[1] == 40
    _assert_equals_batches(s, parts, 40)
    assert s["sim"] == (S0 + s["n_turns"] * N_SIMS) & 0xFFFFFFFF


def test_stream_guards(nets):
    engine = nets[0]
    m = _engine(nets)
    e = engine.SelfPlayEngine(m)
    with pytest.raises(ValueError):
        e.play_stream(N_SIMS, 0)
    with pytest.raises(ValueError):
        e.play_stream(N_SIMS, engine.STREAM_REC_BYTES // (128 * 64 * 4) + 1)
    m.close()


def test_batch_loop_path_gives_the_same_result(nets, stream):
    """Where the one launch does not apply (here: the engine keeps a z_log), play_stream plays the batch loop itself:
    the same result, row for row -- the rows after a game's end included -- and the same sim_counter."""
    s = _stream(nets, z_log_rows=1)
    assert s["launches"] == 3
    for k in ("own", "opp", "valid", "move", "pi", "z", "final_p1", "final_p2", "game_turns", "n_turns", "sim"):
        assert np.array_equal(s[k], stream[k]), k
    for k in stream["tuples"]:
        assert np.array_equal(s["tuples"][k], stream["tuples"][k]), k


def test_a_full_pool_replays_the_stream(nets, monkeypatch):
    """The launch cannot compact its pools: when one fills up, nothing of the attempt counts and the games are played
    again through the batch loop (whose searches compact) -- the same games."""
    engine, ops, policy, value, rw = nets
    G, n, n_sims = 16, 24, 60

    def play(cap):
        m = engine.BatchedMCTS(G, policy, value, rw, n_thr=15, capacity=cap, seed=9, persistent=True)
        e = engine.SelfPlayEngine(m)
        r = e.play_stream(n_sims, n)
        out = {k: getattr(r, k).cpu().numpy() for k in ("own", "opp", "valid", "move", "pi", "z")}
        out.update(n_turns=r.n_turns, launches=r.launches, replayed=getattr(e, "n_replayed", 0), sim=m.sim_counter,
                   leaf=m.n_leaf_evals, turns=r.game_turns.cpu().numpy())
        m.close()
        return out

    want = play(engine.suggest_capacity(n_sims, 15))
    assert want["launches"] == 1 and want["replayed"] == 0
    monkeypatch.setattr(engine, "suggest_capacity", lambda *a, **k: 64)
    got = play(256)
    assert got["launches"] == 2 and got["replayed"] >= 1
    for k in ("own", "opp", "valid", "move", "pi", "z", "turns", "n_turns", "sim"):
        assert np.array_equal(got[k], want[k]), k
