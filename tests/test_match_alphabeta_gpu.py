"""Matches against the fixed-depth alpha-beta opponent (SelfPlayEngine.play_match(opponent=AlphaBeta(d), opening_turns=,
paired=)) with the shipped nets: the records replayed on the CPU rules, every opening move the reference's draw, every
opponent move the reference's search, the pairing, the score, determinism, the negamax backup, and the match with the
new arguments at their defaults."""
import os

import numpy as np
import pytest
import torch

from . import alphabeta_ref as ab
from . import endgame_ref as er

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
B, N_SIMS, N_THR, DEPTH, OPENING, SEED, BASE = 16, 24, 15, 2, 4, 21, 500
START_OWN, START_OPP = 0x0000000810000000, 0x0000001008000000
KEYS = ("own", "opp", "valid", "move", "pi", "z", "final_p1", "final_p2", "mcts_colour")


@pytest.fixture(scope="module")
def nets():
    from iago_amd import network, ops
    policy = network.SLPolicy().load_npz(os.path.join(GOLDEN, "sl_model.npz")).cuda().eval()
    value = network.Value().load_npz(os.path.join(GOLDEN, "value_model.npz")).cuda().eval()
    rollout = network.RolloutPolicy().load_npz(os.path.join(GOLDEN, "rollout_model.npz")).eval()
    return policy, value, ops.RolloutWeights(*rollout.kernel_weights())


def _match(nets, backup=None, **kw):
    from iago_amd import engine
    extra = {} if backup is None else dict(backup=backup)
    m = engine.BatchedMCTS(B, *nets, lmbda=0.5, c_puct=1.0, n_thr=N_THR, seed=SEED, game_id_base=BASE, persistent=True,
                           capacity=engine.suggest_capacity(N_SIMS, N_THR, moves=64), **extra)
    r = engine.SelfPlayEngine(m).play_match(N_SIMS, **kw)
    out = {k: getattr(r, k).cpu().numpy() for k in KEYS}
    out.update(n_turns=r.n_turns, launches=r.launches, sim=m.sim_counter, score=r.score(),
               tuples={k: v.cpu().numpy() for k, v in r.tuples().items()})
    m.close()
    return out


@pytest.fixture(scope="module")
def yard(nets):
    from iago_amd.engine import AlphaBeta
    return _match(nets, opponent=AlphaBeta(DEPTH), opening_turns=OPENING, paired=True)


def _u(x):
    return int(np.uint64(x))


def test_records_replay_on_the_cpu_rules(yard):
    s = yard
    T = s["n_turns"]
    assert s["launches"] == T and s["sim"] == (T * N_SIMS) & 0xFFFFFFFF
    assert s["mcts_colour"].tolist() == [1] * (B // 2) + [2] * (B // 2)
    kinds = {1: 0, 2: 0, 5: 0}
    opponent_rows = 0
    for g in range(B):
        own, opp = START_OWN, START_OPP
        mc = int(s["mcts_colour"][g])
        for t in range(T):
            v, mv = int(s["valid"][t, g]), int(s["move"][t, g])
            assert (_u(s["own"][t, g]), _u(s["opp"][t, g])) == (own, opp), (g, t)
            moves = ab.moves_of(own, opp)
            mover = 1 if t % 2 == 0 else 2
            if v == 0:
                assert mv == -1
                own, opp = opp, own
                continue
            kinds[v] += 1
            assert mv in moves, (g, t, v)
            pi = s["pi"][t, g]
            if v == 5:
                assert t < OPENING and mv == ab.random_move(own, opp, SEED, g, BASE, B // 2, t), (g, t)
                assert not pi.any()
            elif v == 2:
                assert t >= OPENING and not pi.any()
                if mover != mc:
                    opponent_rows += 1
                    assert mv == ab.alphabeta(own, opp, DEPTH)[1], (g, t)
                else:   # PV-MCTS plays without a search only the final only move
                    assert len(moves) == 1 and bin(own | opp).count("1") > 62
            else:
                assert v == 1 and t >= OPENING and mover == mc
                assert pi.sum() >= N_SIMS - N_THR and not pi[[a for a in range(64) if a not in moves]].any()
            own, opp = ab.play(own, opp, mv)
        # the final boards and the result
        p1, p2 = (own, opp) if T % 2 == 0 else (opp, own)
        assert (_u(s["final_p1"][g]), _u(s["final_p2"][g])) == (p1, p2)
        assert not er.bit_legal(p1, p2) and not er.bit_legal(p2, p1)
        d = bin(p1).count("1") - bin(p2).count("1")
        assert int(s["z"][g]) == (d > 0) - (d < 0)
    assert kinds[5] == B * OPENING and kinds[1] > B * 20 and opponent_rows > B * 20
    assert (s["tuples"]["pi"].sum(axis=1) >= N_SIMS - N_THR).all() and len(s["tuples"]["move"]) == kinds[1]


def test_pairs_share_their_opening(yard):
    h = B // 2
    assert np.array_equal(yard["move"][:OPENING, :h], yard["move"][:OPENING, h:])
    assert (yard["valid"][:OPENING] == 5).all() and not (yard["valid"][OPENING:] == 5).any()
    assert (yard["mcts_colour"][:h] == 1).all() and (yard["mcts_colour"][h:] == 2).all()
    # the openings differ between the pairs
    assert len({tuple(yard["move"][:OPENING, g]) for g in range(h)}) > 1


def test_score_agrees_with_the_final_boards(yard):
    z = yard["z"].astype(int) * np.where(yard["mcts_colour"] == 1, 1, -1)
    sc = yard["score"]
    assert (sc["wins"], sc["draws"], sc["losses"], sc["n"]) == ((z > 0).sum(), (z == 0).sum(), (z < 0).sum(), B)
    assert sc["win_rate"] == (sc["wins"] + 0.5 * sc["draws"]) / B


def test_two_runs_give_identical_records(nets, yard):
    from iago_amd.engine import AlphaBeta
    again = _match(nets, opponent=AlphaBeta(DEPTH), opening_turns=OPENING, paired=True)
    for k in KEYS:
        assert np.array_equal(again[k], yard[k]), k
    assert again["n_turns"] == yard["n_turns"] and again["score"] == yard["score"]


def test_negamax_backup_plays_the_match_to_the_end(nets, yard):
    from iago_amd.engine import AlphaBeta
    s = _match(nets, backup="negamax", opponent=AlphaBeta(DEPTH), opening_turns=OPENING, paired=True)
    assert s["score"]["n"] == B and s["launches"] == s["n_turns"]
    assert np.array_equal(s["move"][:OPENING], yard["move"][:OPENING])      # the openings owe nothing to the search
    for g in range(B):
        p1, p2 = _u(s["final_p1"][g]), _u(s["final_p2"][g])
        assert not er.bit_legal(p1, p2) and not er.bit_legal(p2, p1)


def test_defaults_are_the_match_as_it_was(nets):
    plain = _match(nets)
    named = _match(nets, opponent=None, opening_turns=0, paired=False)
    two = _match(nets, mcts_colour=2)
    assert plain["launches"] == named["launches"] == two["launches"]
    for k in KEYS:
        assert np.array_equal(plain[k], named[k]) and np.array_equal(plain[k], two[k]), k
    assert not (plain["valid"] == 5).any() and (plain["mcts_colour"] == 2).all()


def test_openings_alone_keep_the_policy_opponent(nets):
    s = _match(nets, opening_turns=2)
    assert s["launches"] == s["n_turns"] > 1
    assert (s["valid"][:2] == 5).all() and (s["valid"][2:] != 5).all() and (s["valid"][2:] == 2).sum() > B * 20
    want = [ab.random_move(START_OWN, START_OPP, SEED, g, BASE, B, 0) for g in range(B)]
    assert s["move"][0].tolist() == want
