"""Matches: PV-MCTS against the SL policy it is built on (SelfPlayEngine.play_match) -- the reference's `game.py --auto`
(game.py:96-145,246-262) for a batch of games, in ONE persistent launch (iago_mcts_search_args.active 2 / 3) or through
the turn loop.  What must hold: the two paths (and the role split) give the same games record for record; every record
obeys the rules (the C oracle); every policy move is the masked draw of the net's distribution with the match's own
Philox key; a final move that is the only one is played without a search; PV-MCTS's searches are the reference's
(oracle/mcts_py.MCTS, fed both sides' moves); score() and tuples() read the result from PV-MCTS's side."""
import contextlib
import os

import numpy as np
import pytest
import torch

from oracle import mcts_py
from oracle import oracle as orc
from tests.bench_batch_util import replay_match

pytestmark = pytest.mark.gpu

G, N_SIMS, SEED, BASE, S0 = 64, 24, 11, 300, 1000
MATCH_SEED = SEED ^ (0x4D415443 << 32)


@pytest.fixture(scope="module")
def nets():
    from iago_amd import engine, network, ops
    assert torch.cuda.is_available()
    torch.manual_seed(3)
    policy = network.SLPolicy().cuda().eval()          # random init: broad trees
    value = network.Value().cuda().eval()
    # (uniform rollouts: the oracle plays every leaf's rollout itself from the playout's Philox stream)
    return engine, ops, policy, value, ops.uniform_weights()


@contextlib.contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _engine(nets, **kw):
    engine, ops, policy, value, rw = nets
    m = engine.BatchedMCTS(G, policy, value, rw, n_thr=15, capacity=4096, seed=SEED, game_id_base=BASE,
                           persistent=True, **kw)
    m.sim_counter = S0
    return m


def _mixed():
    c = torch.full((G,), 2, dtype=torch.int64, device="cuda")
    c[1::2] = 1                                         # odd games: PV-MCTS moves first
    return c


def _match(nets, colours, loop=False, **kw):
    engine = nets[0]
    m = _engine(nets, **kw)
    with _env(IAGO_PERSISTENT_GAMES="0" if loop else "1"):
        r = engine.SelfPlayEngine(m).play_match(N_SIMS, mcts_colour=colours)
    out = {k: getattr(r, k).cpu().numpy() for k in ("own", "opp", "valid", "move", "pi", "z", "final_p1", "final_p2",
                                                      "mcts_colour")}
    turns = r.game_turns if r.game_turns is not None else engine._end_turns(r.valid)
    out.update(game_turns=turns.cpu().numpy(), n_turns=r.n_turns, launches=r.launches, sim=m.sim_counter,
               split=m._split is not None, score=r.score(), ctl3=int(m._ps["ctl"][3].item()))
    out["tuples"] = {k: v.cpu().numpy() for k, v in r.tuples().items()}
    m.close()
    return out


@pytest.fixture(scope="module")
def mixed(nets):
    return _match(nets, _mixed())


@pytest.fixture(scope="module")
def all2(nets):
    return _match(nets, 2)


KEYS = ("own", "opp", "valid", "move", "pi", "z", "final_p1", "final_p2", "game_turns", "n_turns", "sim")


@pytest.mark.parametrize("which", ["mixed", "all2"])
def test_one_launch_equals_the_turn_loop(nets, mixed, all2, which):
    one = mixed if which == "mixed" else all2
    loop = _match(nets, _mixed() if which == "mixed" else 2, loop=True)
    assert one["launches"] == 1 and one["ctl3"] == 0 and loop["launches"] == loop["n_turns"] > 1
    for k in KEYS:
        assert np.array_equal(one[k], loop[k]), k
    assert one["sim"] == (S0 + one["n_turns"] * N_SIMS) & 0xFFFFFFFF
    # both kinds of move are there, on both sides
    assert (one["valid"] == 1).sum() > G * 20 and (one["valid"] == 2).sum() > G * 20


def test_role_split_plays_the_same_match(nets, mixed):
    s = _match(nets, _mixed(), split=8)
    if not s["split"]:
        pytest.skip("this runtime gives no CU-masked streams")
    assert s["launches"] == 1 and s["ctl3"] == 0
    for k in KEYS:
        assert np.array_equal(s[k], mixed[k]), k


def _bits(x):
    return x.view(np.uint64)                            # (bit 63 set: a negative int64)


def _replay(s, g, on_turn=None):
    """Game g of result s through the C oracle, every record checked (tests/bench_batch_util.replay_match)."""
    return replay_match(s, g, N_SIMS, on_turn=on_turn)


@pytest.mark.parametrize("which", ["mixed", "all2"])
def test_match_records_follow_the_rules(mixed, all2, which):
    s = mixed if which == "mixed" else all2
    n = sum(_replay(s, g) for g in range(G))
    assert n == int(s["game_turns"].sum())
    assert s["valid"].shape[0] == s["n_turns"] == int(s["game_turns"].max())


def test_policy_moves_are_the_masked_draws(nets, mixed, all2):
    """Every policy move: orc_choice_cdf over the masked distribution (game.py:100-104) of forward_boards_split3 on the
    recorded position, with the uniform of (seed ^ 0x4D415443 << 32, game_id_base + g, turn, stream 0)."""
    ops, policy = nets[1], nets[2]
    n = 0
    for s in (mixed, all2):
        rows = []
        for g in range(G):
            def hook(t, state, color, kind, acts, g=g):
                if kind == "draw":
                    rows.append((t, g, list(acts)))
            _replay(s, g, hook)
        own = torch.tensor(np.array([s["own"][t, g] for t, g, _ in rows]), device="cuda")
        opp = torch.tensor(np.array([s["opp"][t, g] for t, g, _ in rows]), device="cuda")
        probs = policy.forward_boards_split3(own, opp).cpu().numpy().reshape(-1, 64)
        for (t, g, acts), prob in zip(rows, probs):
            u = orc.uniform(MATCH_SEED, BASE + g, t, 0)
            want = orc.choice_cdf(orc.masked_probs(prob, acts), u)
            assert int(s["move"][t, g]) == want, (t, g)
        n += len(rows)
    assert n > 2 * G * 20


def test_forced_final_moves(mixed, all2):
    """A mover with 63 stones on the board and one legal move plays it without a search (game.py:97-98): valid 2, pi 0,
    on either side; the batch has such rows."""
    n = 0
    for s in (mixed, all2):
        own, opp = _bits(s["own"]), _bits(s["opp"])
        for g in range(G):
            for t in range(int(s["game_turns"][g])):
                o, p = int(own[t, g]), int(opp[t, g])
                if bin(o | p).count("1") != 63:
                    continue
                st = orc.bits_to_state(o, p)
                if len(orc.legal_actions(st, 1)) == 1:
                    assert s["valid"][t, g] == 2 and not s["pi"][t, g].any(), (g, t)
                    n += 1
    assert n > 0


def test_searches_match_the_oracle(nets, mixed):
    """PV-MCTS's first three searches in games of both colours: the root's visit counts as oracle/mcts_py.MCTS builds
    them, fed the same nets (the production kernels on one board), the rollouts of the same Philox streams (stream
    sim_counter + turn x n_sims + playout) and update_with_move for BOTH sides' moves -- tree reuse across the policy's
    move included."""
    from tests.test_mcts_production_gpu import NetProbe
    engine, ops, policy, value, _ = nets
    probe = NetProbe(ops, policy, value)
    s = mixed
    for g in (0, 1, 2, 3):
        counter = [0]

        def roll(state, color, g=g, counter=counter):
            z = orc.random_playout(state, color, seed=SEED, game_id=BASE + g, stream=counter[0])[0]
            counter[0] += 1
            return z

        om = mcts_py.MCTS(probe.policy_fn, probe.value_fn, roll, lmbda=0.5, c_puct=1.0, n_thr=15)
        done = [0]

        def hook(t, state, color, kind, acts, g=g, om=om, counter=counter, done=done):
            a = int(s["move"][t, g])
            if done[0] >= 3:
                return
            if kind == "search":
                counter[0] = S0 + t * N_SIMS
                got = om.get_move(np.array(state, dtype=np.float32), color, N_SIMS)
                want = np.zeros(64, np.int64)
                for b, ch in om.root.children.items():
                    if b >= 0:
                        want[b] = ch.n_visits
                assert np.array_equal(want, s["pi"][t, g]), (g, t)
                assert got == a, (g, t)
                done[0] += 1
            if kind != "forced":
                om.update_with_move(a)      # (a pass: -1)

        _replay(s, g, hook)
        assert done[0] == 3, g


def test_score_tuples_and_arguments(nets, mixed, all2):
    engine = nets[0]
    for s, col in ((mixed, np.where(np.arange(G) % 2 == 1, 1, 2)), (all2, np.full(G, 2))):
        assert np.array_equal(s["mcts_colour"], col)
        zm = s["z"].astype(np.int64) * np.where(col == 1, 1, -1)
        sc = s["score"]
        assert (sc["wins"], sc["draws"], sc["losses"], sc["n"]) == \
            (int((zm > 0).sum()), int((zm == 0).sum()), int((zm < 0).sum()), G)
        assert sc["win_rate"] == pytest.approx((sc["wins"] + 0.5 * sc["draws"]) / G)
        tp = s["tuples"]
        t, g = tp["turn"], tp["game"] - BASE
        assert len(t) == int((s["valid"] == 1).sum())
        assert np.all(s["valid"][t, g] == 1)
        assert np.array_equal(tp["colour"], col[g]) and np.array_equal(tp["move"], s["move"][t, g])
        assert np.array_equal(tp["pi"], s["pi"][t, g])
    m = _engine(nets)
    e = engine.SelfPlayEngine(m)
    bad = [0, 3, True, 1.0, torch.full((G - 1,), 2, device="cuda"), torch.full((G, 1), 2, device="cuda"),
           torch.zeros(G, dtype=torch.int64, device="cuda"), torch.full((G,), 3, dtype=torch.int64, device="cuda"),
           torch.full((G,), 2.0, device="cuda")]
    for c in bad:
        with pytest.raises(ValueError):
            e.play_match(N_SIMS, mcts_colour=c)
    m.close()
