"""The role split at the sizes where it is the engine's default, against the oracle.

BatchedMCTS splits the persistent search by role (iago_mcts_search_split: the game workgroups two per CU on a CU-masked
stream, the net workgroups on the other CUs) for every batch of more than 32 game workgroups -- every batch above 1024
games.  2048 games take 32 game CUs and leave 224 net workgroups, 4096 games 64 and 192: the batches bench.py's
`mcts_saturated` leg times.  Only there do game ids >= 1024 exist (their rows of every per-game array, their Philox
keys, their writer tags in the position table), two game workgroups share a CU and 224 net workgroups serve the rings.
Each fixture below is ONE launch on an engine built as bench.py builds its engines (random-init nets, seed 0; shipped
rollout weights; engine seed 7; suggest_capacity; z_log on where the launch allows it), and

  A  2048 whole games x 100 playouts: record for record the single launch (split=0); every record through the C
     oracle; searches of games on both halves, both workgroups of a CU pair and the edges of a workgroup, and two whole
     games, rebuilt by oracle/mcts_py.MCTS; the position table audited;
  B  4096 whole games x 100 playouts: every record through the oracle, searches of 8 games rebuilt, the table audited;
  C  1100 games x 60 playouts (35 game workgroups, the last one of 12 games): record for record the single launch,
     games 1024-1099 and a sample through the oracle;
  D  2048 games x 24 playouts, uniform rollouts, ids 64512 .. 66559 (across 2^16): 6 whole games played by the oracle
     itself, every rollout drawn from the Philox stream (seed, game id, turn x n_sims + playout) -- nothing replayed;
  E  a stream of 2560 games through 2048 slots in one split launch: games 0-2047 are A's, games 2048-2559 pass the
     oracle;
  F  a match of 2048 games, split against single launch record for record, the same score, every record by the rules.

Every split launch: the split engaged with the workgroup counts that follow from the device, not given up, nothing
replayed, no pool overflow (test_launch_shape; `-s` prints the counts).
"""
import time

import numpy as np
import pytest
import torch

from oracle import mcts_py
from oracle import oracle as orc
from tests.bench_batch_util import (Probe, audit_table, make_nets, rebuild_in_workers, replay_match, replay_records)
from tests.conftest import load_json

pytestmark = pytest.mark.gpu

N_THR, SEED, GPW = 15, 7, 32
D_BASE = 65536 - 1024          # D: game ids cross 2^16 half-way through the batch


@pytest.fixture(scope="module")
def nets():
    from iago_amd import engine, ops
    assert torch.cuda.is_available()
    policy, value = make_nets()                        # bench.mcts_leg's nets: random init, seed 0
    g = load_json("simulate.json")
    return engine, ops, policy, value, ops.RolloutWeights(g["shipped_w"], g["shipped_b"])


def _engine(nets, n_games, n_sims, z_log=True, uniform=False, base=0, **kw):
    engine, ops, policy, value, shipped = nets
    m = engine.BatchedMCTS(n_games, policy, value, ops.uniform_weights() if uniform else shipped, lmbda=0.5, c_puct=1.0,
                           n_thr=N_THR, seed=SEED, game_id_base=base, persistent=True,
                           z_log_rows=128 * n_sims if z_log else 0,
                           capacity=engine.suggest_capacity(n_sims, N_THR, moves=64), **kw)
    assert m.persistent and m.value_cache and m.games_per_workgroup == GPW
    m.warmup()
    return m, engine.SelfPlayEngine(m, max_turns=128)


def _snap(nets, m, eng, res, n_sims, table=False):
    """The launch's result, its workgroup counts and control words as host arrays (tests/bench_batch_util's layout)."""
    ops = nets[1]
    B = dict(ops=ops, policy=nets[2], value=nets[3], n_sims=n_sims, n_thr=m.n_thr, T=res.n_turns,
             path_stride=m.PATH_STRIDE, n_games=len(res.z),
             own=ops.tensor_to_bits(res.own), opp=ops.tensor_to_bits(res.opp),
             valid=res.valid.cpu().numpy(), move=res.move.cpu().numpy(), pi=res.pi.cpu().numpy(),
             z=res.z.cpu().numpy(), game_turns=res.game_turns.cpu().numpy(),
             f1=ops.tensor_to_bits(res.final_p1), f2=ops.tensor_to_bits(res.final_p2),
             leaf_evals=m.n_leaf_evals, launches=getattr(res, "launches", 1),
             slots=m.n_games, split=m._split is not None, split_cus=m.split_cus, net_workgroups=m.net_workgroups,
             resident=m.resident_workgroups, gpw=m.games_per_workgroup, launched=m.net_workgroups_launched,
             ctl=[int(x) for x in m._ps["ctl"].tolist()], replayed=getattr(eng, "n_replayed", 0),
             overflow=int(m.tree.overflow.sum().item()))
    B["final_p1"], B["final_p2"] = B["f1"], B["f2"]
    if getattr(res, "mcts_colour", None) is not None:
        B["mcts_colour"] = res.mcts_colour.cpu().numpy()
        B["score"] = res.score()
    if m.z_log is not None:
        B["zlog"], B["zn"] = m.z_log.cpu().numpy(), m.z_log_n.cpu().numpy()
    if table:
        B["table"] = m._vtable.cpu().numpy().view(np.uint64).reshape(-1, 4)
    return B


def _self_play(nets, n_games, n_sims, table=False, **kw):
    m, eng = _engine(nets, n_games, n_sims, **kw)
    t0 = time.time()
    res = eng.play(n_sims, record=True)
    B = _snap(nets, m, eng, res, n_sims, table=table)
    B["wall_s"] = time.time() - t0
    m.close()
    return B


@pytest.fixture(scope="module")
def a_split(nets):
    return _self_play(nets, 2048, 100, table=True)


@pytest.fixture(scope="module")
def a_single(nets):
    return _self_play(nets, 2048, 100, split=0)


@pytest.fixture(scope="module")
def b_split(nets):
    return _self_play(nets, 4096, 100, table=True)


@pytest.fixture(scope="module")
def c_split(nets):
    return _self_play(nets, 1100, 60)


@pytest.fixture(scope="module")
def c_single(nets):
    return _self_play(nets, 1100, 60, split=0)


@pytest.fixture(scope="module")
def d_split(nets):
    return _self_play(nets, 2048, 24, uniform=True, base=D_BASE)


@pytest.fixture(scope="module")
def e_stream(nets):
    # (no z_log: a stream refuses it -- its rows are slots, its games many more)
    m, eng = _engine(nets, 2048, 100, z_log=False)
    res = eng.play_stream(100, 2560)
    B = _snap(nets, m, eng, res, 100)
    m.close()
    return B


def _match(nets, **kw):
    m, eng = _engine(nets, 2048, 100, **kw)
    res = eng.play_match(100)
    B = _snap(nets, m, eng, res, 100)
    m.close()
    return B


@pytest.fixture(scope="module")
def f_split(nets):
    return _match(nets)


@pytest.fixture(scope="module")
def f_single(nets):
    return _match(nets, split=0)


LAUNCHES = dict(a_split=(2048, True), a_single=(2048, False), b_split=(4096, True), c_split=(1100, True),
                c_single=(1100, False), d_split=(2048, True), e_stream=(2048, True), f_split=(2048, True),
                f_single=(2048, False))


@pytest.mark.parametrize("name", list(LAUNCHES))
def test_launch_shape(request, name):
    """One launch, not given up, nothing replayed, no pool overflow; where the split is the default, the split engaged
    with 8 game CUs per 16 game workgroups and one net workgroup on every other CU (at most 7/8 of the device's)."""
    B = request.getfixturevalue(name)
    slots, split = LAUNCHES[name]
    ctl = B["ctl"]
    assert B["slots"] == slots and B["gpw"] == GPW
    assert B["launches"] == 1 and B["replayed"] == 0 and B["overflow"] == 0
    assert ctl[3] == 0 and ctl[4] == 0, ctl                  # not given up; every searched root had children
    if "mcts_colour" in B:
        assert ctl[13] == 0, ctl                             # no policy draw without mass on the legal moves
    n_gw = -(-slots // GPW)
    print("%s: %d slots, %d game workgroups, split %s, split_cus %d, net workgroups %d (launched %d), resident %d, "
          "%d turns, %.1f s" % (name, slots, n_gw, B["split"], B["split_cus"], B["net_workgroups"], B["launched"],
                                B["resident"], B["T"], B.get("wall_s", float("nan"))))
    if not split:
        assert not B["split"] and B["split_cus"] == 0
        return
    if not B["split"]:
        pytest.skip("this runtime gives no CU-masked streams")
    assert B["split_cus"] == 8 * -(-n_gw // 16)
    assert B["net_workgroups"] == B["resident"] - max(B["split_cus"], B["resident"] // 8)
    assert ctl[7] == B["net_workgroups"] == B["launched"]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert B["resident"] % cus == 0 and B["split_cus"] <= cus // 2


def test_split_argument(nets):
    """split= must be "auto", 0 or a positive multiple of 8 (a value that can never split raised nothing and took the
    single launch); split=8 at 2048 games is widened to the 32 CUs its 64 game workgroups need."""
    engine, ops, policy, value, _ = nets
    for bad in (True, 12, -8, "x"):
        with pytest.raises(ValueError):
            engine.BatchedMCTS(2048, policy, value, ops.uniform_weights(), persistent=True, split=bad)
    m = engine.BatchedMCTS(2048, policy, value, ops.uniform_weights(), persistent=True, capacity=1024, split=8)
    if m._split is None:
        m.close()
        pytest.skip("this runtime gives no CU-masked streams")
    assert m.split_cus == 32
    m.close()


REC = ("own", "opp", "valid", "move", "pi", "z", "game_turns", "f1", "f2")


def _assert_same_records(x, y, keys=REC):
    assert x["T"] == y["T"]
    for k in keys:
        assert np.array_equal(x[k], y[k]), k


# ---------------------------------------------------------------- A: 2048 whole games x 100 playouts

def test_a_equals_the_single_launch(a_split, a_single):
    _assert_same_records(a_split, a_single, REC + ("zlog", "zn"))
    assert a_split["leaf_evals"] == a_single["leaf_evals"] == int(a_split["valid"].sum()) * 100


def test_a_records_through_the_oracle(a_split):
    t0 = time.time()
    n = replay_records(a_split, whole=True)
    print("A: %d records through the oracle in %.1f s" % (n, time.time() - t0))
    assert n > 2048 * 58


def test_a_searches_rebuilt_by_the_oracle(a_split, tmp_path):
    """The first 4 searches of games on both halves, both workgroups of a CU pair (0-31, 32-63) and the first and last
    slot of a workgroup; two whole games, one of them >= 1024."""
    B = a_split
    firsts = (0, 31, 32, 1023, 1024, 1055, 2016, 2047)
    jobs = [(g, 4, 0) for g in firsts] + [(g, 128, 0) for g in (700, 1500)]
    n_cmp, depth = rebuild_in_workers(B, jobs, tmp_path)
    assert n_cmp >= len(firsts) * 4 + 2 * 55
    assert len(depth) == 10 and max(depth.values()) < B["path_stride"]


def _audit(B):
    used, walked = audit_table(B, 4096)
    writer = (B["table"][:, 0][np.nonzero(B["table"][:, 0])[0]] >> np.uint64(32)).astype(np.int64)
    assert writer.max() >= 1024                                # an entry written by a game of the upper half
    return used, walked


def test_a_position_table_audit(a_split):
    used, walked = _audit(a_split)
    assert used > 200_000 and walked == 4096


# ---------------------------------------------------------------- B: 4096 whole games x 100 playouts

def test_b_records_through_the_oracle(b_split):
    n = replay_records(b_split, whole=True)
    assert n > 4096 * 58 and b_split["leaf_evals"] == int(b_split["valid"].sum()) * 100


def test_b_searches_rebuilt_by_the_oracle(b_split, tmp_path):
    jobs = [(g, 4, 0) for g in (0, 777, 1023, 1024, 2047, 2048, 3333, 4095)]
    n_cmp, _ = rebuild_in_workers(b_split, jobs, tmp_path)
    assert n_cmp == 8 * 4


def test_b_position_table_audit(b_split):
    used, walked = _audit(b_split)
    writer = (b_split["table"][:, 0][np.nonzero(b_split["table"][:, 0])[0]] >> np.uint64(32)).astype(np.int64)
    assert writer.max() >= 2048 and used > 200_000 and walked == 4096


# ---------------------------------------------------------------- C: ragged split, 1100 games x 60 playouts

def test_c_ragged_split_equals_the_single_launch(c_split, c_single):
    """35 game workgroups, the last one of 12 games (34 x 32 + 12)."""
    assert -(-1100 // GPW) == 35 and 1100 - 34 * GPW == 12
    _assert_same_records(c_split, c_single, REC + ("zlog", "zn"))
    games = list(range(1024, 1100)) + list(range(0, 1024, 97))
    assert replay_records(c_split, whole=True, games=games) > len(games) * 58


# ---------------------------------------------------------------- D: Philox keys above 1024, nothing replayed

def test_d_oracle_plays_the_games_itself(nets, d_split):
    """Uniform rollouts: the oracle plays every rollout from the Philox stream of (seed, D_BASE + g, turn x n_sims +
    playout) -- game ids 64512 .. 66559 -- with its own MCTS.py restatement: the same root visit counts, moves, results
    and final boards."""
    B = d_split
    n_sims = B["n_sims"]
    probe = Probe(B)
    for g in (0, 511, 1023, 1024, 1500, 2047):
        counter = [0]

        def roll(state, color, g=g, counter=counter):
            z = orc.random_playout(state, color, seed=SEED, game_id=D_BASE + g, stream=counter[0])[0]
            counter[0] += 1
            return z

        om = mcts_py.MCTS(probe.policy_fn, probe.value_fn, roll, lmbda=0.5, c_puct=1.0, n_thr=N_THR)
        state = orc.initial_state()
        stone_num, pass_flg, t = 4, False, 0
        while stone_num < 64:                              # game.py:117-142,253-255
            for color in (1, 2):
                acts = orc.legal_actions(state, color)
                if len(acts) > 0:
                    counter[0] = t * n_sims
                    a = om.get_move(state, color, n_sims)
                    want = np.zeros(64, np.int64)
                    for act, ch in om.root.children.items():
                        want[act] = ch.n_visits
                    assert B["valid"][t, g] == 1 and int(B["move"][t, g]) == a, (g, t)
                    assert B["pi"][t, g].tolist() == want.tolist(), (g, t)
                    om.update_with_move(a)
                    orc.place_stone(state, a, color)
                    stone_num += 1
                    pass_flg = False
                else:
                    assert B["valid"][t, g] == 0 and B["move"][t, g] == -1, (g, t)
                    if pass_flg:
                        stone_num = 64
                    pass_flg = True
                    om.update_with_move(-1)
                t += 1
        assert int(B["game_turns"][g]) == t, g
        assert B["z"][g] == orc.judge(state, 1) and orc.state_to_bits(state) == (int(B["f1"][g]), int(B["f2"][g])), g


# ---------------------------------------------------------------- E: a stream at 2048 slots

def test_e_stream_at_2048_slots(e_stream, a_split):
    """play_stream(100, 2560) on 2048 slots: games 0-2047 are A's batch (batch 0 of the batch loop), the 512 games the
    slots claimed after their first game pass the oracle."""
    S, A = e_stream, a_split
    assert S["n_games"] == 2560 and S["T"] == int(S["game_turns"].max())
    for g in range(2048):
        t = int(A["game_turns"][g])
        assert int(S["game_turns"][g]) == t, g
        for k in ("z", "f1", "f2"):
            assert S[k][g] == A[k][g], (g, k)
        for k in ("own", "opp", "valid", "move", "pi"):
            assert np.array_equal(S[k][:t, g], A[k][:t, g]), (g, k)
    assert replay_records(S, whole=True, games=range(2048, 2560)) > 512 * 58


# ---------------------------------------------------------------- F: a match at 2048 games

def test_f_match_split_equals_single_launch(f_split, f_single):
    _assert_same_records(f_split, f_single, REC + ("zlog", "zn", "mcts_colour"))
    assert f_split["score"] == f_single["score"] and f_split["score"]["n"] == 2048


def test_f_match_records_follow_the_rules(f_split):
    s = f_split
    n = sum(replay_match(s, g, s["n_sims"], n_thr=N_THR) for g in range(2048))
    assert n == int(s["game_turns"].sum())
    assert (s["valid"] == 1).sum() > 2048 * 20 and (s["valid"] == 2).sum() > 2048 * 20
