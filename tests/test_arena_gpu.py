"""ArenaEngine (engine.py): whole games between two PV-MCTS agents with their own nets.  What must hold: one launch per
turn (iago_mcts_search_arena) and the sequential form (mcts_a.search, then mcts_b.search) play the same games record for
record; every record obeys the rules (the C oracle, turn by turn, as tests/bench_batch_util.replay_match walks a match --
whose kinds of move, a policy draw and a forced final move, an arena game does not have: every mover with a move
searches); `agent` follows the colour rule and `pi` is zero where nobody searched; explored openings are the mover's
draw (tests/explore_ref.py) under the mover's seed and id; tuples(agent=) partition tuples() and go into a replay
window unchanged."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import explore_ref
from tests.conftest import load_json

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

G, N_SIMS, N_THR = 16, 16, 2     # (n_thr 2: at the default 15 no root expands in 16 playouts)
SEED = dict(a=11, b=12)
BASE = dict(a=300, b=9000)
S0 = dict(a=1000, b=4000)
RECORDS = ("own", "opp", "valid", "move", "pi", "agent", "z", "final_p1", "final_p2", "a_colour")


@pytest.fixture(scope="module")
def nets():
    from iago_amd import engine, network, ops
    assert torch.cuda.is_available()
    pairs = {}
    for name, seed in (("a", 3), ("b", 4)):
        torch.manual_seed(seed)
        pairs[name] = (network.SLPolicy().cuda().eval(), network.Value().cuda().eval())
    g = load_json("simulate.json")
    return engine, ops, pairs, ops.RolloutWeights(g["shipped_w"], g["shipped_b"])


def _play(nets, one_launch, a_colour=None, lmbda=0.5, n_sims=N_SIMS, **kw):
    engine, ops, pairs, rw = nets
    ms = {}
    for who in ("a", "b"):
        ms[who] = engine.BatchedMCTS(G, pairs[who][0], pairs[who][1], rw, n_thr=N_THR, lmbda=lmbda,
                                     capacity=engine.suggest_capacity(max(np.atleast_1d(n_sims)), N_THR), seed=SEED[who],
                                     game_id_base=BASE[who], persistent=True)
        ms[who].sim_counter = S0[who]
    arena = engine.ArenaEngine(ms["a"], ms["b"])
    r = arena.play(n_sims, a_colour=a_colour, one_launch=one_launch, **kw)
    out = {k: getattr(r, k).cpu().numpy() for k in RECORDS}
    out.update(n_turns=r.n_turns, launches=r.launches, arena_launches=arena.n_arena_launches, score=r.score(),
               sim_a=ms["a"].sim_counter, sim_b=ms["b"].sim_counter, result=r,
               gave_up=[int(m._ps["ctl"][3].item()) for m in ms.values()])
    return out


def _mixed():
    c = torch.full((G,), 2, dtype=torch.int64, device="cuda")
    c[[0, 3, 4, 9, 10, 11, 15]] = 1
    return c


@pytest.fixture(scope="module")
def games(nets):
    """(colours) -> (one launch per turn, sequential)."""
    return {name: (_play(nets, True, col), _play(nets, False, col)) for name, col in (("halves", None), ("mixed", _mixed()))}


@pytest.mark.parametrize("colours", ["halves", "mixed"])
def test_the_two_forms_play_the_same_games(games, colours):
    one, seq = games[colours]
    for k in RECORDS + ("n_turns", "sim_a", "sim_b", "score"):
        assert np.array_equal(one[k], seq[k]), k
    n = one["n_turns"]
    assert one["gave_up"] == seq["gave_up"] == [0, 0]
    assert one["sim_a"] == S0["a"] + n * N_SIMS and one["sim_b"] == S0["b"] + n * N_SIMS
    # the one-launch form did launch the arena kernel, at every turn at which both agents had movers
    searched = one["valid"] == 1
    a_row, b_row = (searched & (one["agent"] == 0)).any(axis=1), (searched & (one["agent"] == 1)).any(axis=1)
    both = int((a_row & b_row).sum())
    assert one["arena_launches"] == both > 40 and seq["arena_launches"] == 0
    assert seq["launches"] == int(a_row.sum()) + int(b_row.sum()) == one["launches"] + both


def _bits(x):
    return x.view(np.uint64)


def _replay(s, g, on_search=None, argmax=True):
    """Game g through the C oracle's rules (game.py:117-142,253-255 with both colours searching): positions, legal
    moves, passes, the books, the end, the result.  Returns (turns, final state)."""
    own, opp = _bits(s["own"]), _bits(s["opp"])
    ac = int(s["a_colour"][g])
    state = orc.initial_state()
    stone_num, pass_flg, t, over = 4, False, 0, False
    while not over and t < 128:
        for color in (1, 2):
            p1, p2 = orc.state_to_bits(state)
            assert (int(own[t, g]), int(opp[t, g])) == ((p1, p2) if color == 1 else (p2, p1)), (g, t)
            assert int(s["agent"][t, g]) == (0 if color == ac else 1), (g, t)          # the colour rule
            acts = orc.legal_actions(state, color)
            row, a = s["pi"][t, g], int(s["move"][t, g])
            if len(acts) > 0:
                assert s["valid"][t, g] == 1 and a in acts, (g, t, a)
                assert np.all(row[[x for x in range(64) if x not in acts]] == 0), (g, t)
                assert int(row.sum()) >= N_SIMS - N_THR, (g, t)
                if argmax:
                    assert a == int(np.argmax(row)), (g, t)
                if on_search:
                    on_search(t, g, color, row, a, acts)
                orc.place_stone(state, a, color)
                stone_num += 1
                pass_flg = False
            else:
                assert s["valid"][t, g] == 0 and a == -1 and not row.any(), (g, t)      # nobody searched: pi is zero
                if pass_flg:
                    stone_num = 64
                pass_flg = True
            t += 1
        if stone_num >= 64:
            over = True
    assert over and t % 2 == 0
    # (after its end a game records no move until the batch's last game is over)
    assert not s["valid"][t:, g].any() and np.all(s["move"][t:, g] == -1) and not s["pi"][t:, g].any()
    assert s["z"][g] == orc.judge(state, 1), g
    assert orc.state_to_bits(state) == (int(_bits(s["final_p1"])[g]), int(_bits(s["final_p2"])[g])), g
    return t


@pytest.mark.parametrize("colours", ["halves", "mixed"])
def test_records_follow_the_rules_and_the_colour_rule(games, colours):
    s = games[colours][0]
    turns = [_replay(s, g) for g in range(G)]
    assert s["n_turns"] == max(turns) == s["valid"].shape[0]
    want = [1] * (G // 2) + [2] * (G // 2) if colours == "halves" else _mixed().cpu().tolist()
    assert s["a_colour"].tolist() == want
    # agent[t, g]: A iff a_colour[g] == (1 if t % 2 == 0 else 2), on every row
    mover = np.where(np.arange(s["n_turns"]) % 2 == 0, 1, 2).reshape(-1, 1)
    assert np.array_equal(s["agent"], (s["a_colour"].reshape(1, G) != mover).astype(np.uint8))
    assert not s["pi"][s["valid"] == 0].any() and np.all(s["pi"][s["valid"] == 1].sum(axis=1) >= N_SIMS - N_THR)
    # score(): A's side of the final boards, recomputed
    p1 = np.array([bin(int(x)).count("1") for x in _bits(s["final_p1"])])
    p2 = np.array([bin(int(x)).count("1") for x in _bits(s["final_p2"])])
    z = np.sign(p1 - p2) * np.where(s["a_colour"] == 1, 1, -1)
    n = dict(wins=int((z > 0).sum()), draws=int((z == 0).sum()), losses=int((z < 0).sum()))
    assert s["score"] == dict(n=G, win_rate=(n["wins"] + 0.5 * n["draws"]) / G, **n)


def test_explored_openings_are_the_movers_draws(nets):
    """explore_turns = 4, lmbda = 0: both forms agree, and each drawn move is explore_ref's draw on the mover's visit row
    with the MOVER's engine's seed and id."""
    one, seq = (_play(nets, form, None, lmbda=0.0, explore_turns=4) for form in (True, False))
    for k in RECORDS + ("n_turns", "sim_a", "sim_b"):
        assert np.array_equal(one[k], seq[k]), k
    seen = []

    def on_search(t, g, color, row, a, acts):
        if t < 4:
            who = "a" if int(one["agent"][t, g]) == 0 else "b"
            assert a == explore_ref.draw(row, SEED[who], BASE[who] + g, t, acts), (t, g, who)
            seen.append((who, a != int(np.argmax(row))))
        else:
            assert a == int(np.argmax(row)), (t, g)

    for g in range(G):
        _replay(one, g, on_search, argmax=False)
    assert {w for w, _ in seen} == {"a", "b"} and any(off for _, off in seen) and len(seen) == 4 * G


def test_tuples_by_agent_partition_the_round(nets, games):
    from iago_amd import network
    from iago_amd.replay import ReplayWindow
    from iago_amd.train_rl import ReinforceTrainer
    r = games["mixed"][0]["result"]
    every, ta, tb = r.tuples(), r.tuples(agent=0), r.tuples(agent=1)
    n = every["own"].numel()
    assert 0 < ta["own"].numel() < n and ta["own"].numel() + tb["own"].numel() == n
    key = lambda t: (t["turn"].to(torch.int64) * (1 << 32) + t["game"].to(torch.int64))
    both = {k: torch.cat([ta[k], tb[k]]) for k in every}
    order = torch.argsort(key(both))
    assert torch.equal(key(both)[order], key(every))           # (tuples(): rows in (turn, game) order, each once)
    for k in every:
        assert torch.equal(both[k][order], every[k]), k
    # A's rows are the rows A moved in
    agent = torch.as_tensor(games["mixed"][0]["agent"], device="cuda")
    assert bool((agent[ta["turn"].long(), (ta["game"] - BASE["a"]).long()] == 0).all())
    assert bool((agent[tb["turn"].long(), (tb["game"] - BASE["a"]).long()] == 1).all())
    model = network.SLPolicy()
    model.load_state_dict(nets[2]["a"][0].state_dict())
    tr = ReinforceTrainer(model, pool_dir=None, N=2, seed=1)
    for tup in (every, ta, tb):
        m = tup["own"].numel()
        w = ReplayWindow(m + 4, seed=1)
        assert tr.add_to_window(w, tup) == m == w.count
        got = w.gather(torch.arange(m), 0)
        order = torch.argsort(key(tup), stable=True)
        for k in ("own", "opp", "pi", "move", "z"):
            assert torch.equal(got[k], tup[k][order].to(got[k].dtype)), k
