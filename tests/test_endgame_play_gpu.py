"""The endgame of self-play and match games played by the exact solver (solve_empties), on the device.

  1  ops.play_endgame (iago_play_endgame) against the host reference tests/endgame_play_ref.py on 512 late positions,
     both parities of `turn`, both pass flags: every record, the turn counts and the final boards bit for bit; every
     solved row equals ops.solve_endgame of its position.
  2  play(100, solve_empties=8) as one launch + play-out against the turn loop (IAGO_PERSISTENT_GAMES=0), record for
     record; the same through the role split at the sizes of tests/test_split_default_sizes_gpu.py -- 2048 games, 4096
     games (64 game CUs), 1100 games x 60 playouts (35 game workgroups, the last one of 12 games) and a stream of 2560
     games through 2048 slots (game ids past the slots); play_stream's game G against game G of the batch loop.
  3  the rows before a game's first solved row are play(100)'s without solve_empties.
  4  every solved row's (score, move) is the C reference solver's; z is the sign of the first solved score; no searched
     row has <= k empties.
  5  play_match(100, solve_empties=8), whole games in one launch allowed (the match stays on the turn loop): PV-MCTS's non-forced late turns are solved, the policy's are not, PV-MCTS's final
     disc difference is at least its first solved score; tuples() holds no solved row.
  6  n_leaf_evals and sim_counter.
Every launch gets the engine's device-clock limits; the positions have at most 10 empties (tens of milliseconds).
"""
import os

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests.bench_batch_util import make_nets
from tests.conftest import load_json

from . import endgame_play_ref as play_ref
from . import endgame_ref as ref

pytestmark = pytest.mark.gpu

N_THR, SEED, K, N_SIMS, T = 15, 7, 8, 100, 128
RECORDS = ("own", "opp", "valid", "move", "pi", "score", "z", "f1", "f2", "game_turns")


@pytest.fixture(scope="module")
def nets():
    from iago_amd import engine, ops
    assert torch.cuda.is_available()
    policy, value = make_nets()
    g = load_json("simulate.json")
    return engine, ops, policy, value, ops.RolloutWeights(g["shipped_w"], g["shipped_b"])


def _engine(nets, n_games, **kw):
    engine, ops, policy, value, shipped = nets
    m = engine.BatchedMCTS(n_games, policy, value, shipped, lmbda=0.5, c_puct=1.0, n_thr=N_THR, seed=SEED,
                           persistent=True, capacity=engine.suggest_capacity(N_SIMS, N_THR, moves=64), **kw)
    assert m.persistent
    m.warmup()
    return m, engine.SelfPlayEngine(m, max_turns=T)


def _snap(nets, m, eng, res):
    ops = nets[1]
    B = dict(own=ops.tensor_to_bits(res.own), opp=ops.tensor_to_bits(res.opp), valid=res.valid.cpu().numpy(),
             move=res.move.cpu().numpy(), pi=res.pi.cpu().numpy(), score=getattr(res, res.SCORE_RECORD).cpu().numpy(), z=res.z.cpu().numpy(),
             f1=ops.tensor_to_bits(res.final_p1), f2=ops.tensor_to_bits(res.final_p2), n_turns=res.n_turns,
             launches=res.launches, sim=m.sim_counter, leaf_evals=m.n_leaf_evals, replayed=eng.n_replayed,
             split=m._split is not None, ctl3=int(m._ps["ctl"][3].item()))
    B["game_turns"] = (res.game_turns if res.game_turns is not None else nets[0]._end_turns(res.valid)).cpu().numpy()
    if getattr(res, "mcts_colour", None) is not None:
        B["mcts_colour"] = res.mcts_colour.cpu().numpy()
        B["tuples_valid"] = int(res.tuples()["own"].numel())
    B["n_solved_tuples"] = int(res.solved_tuples()["score"].numel())
    B["solved_tuples"] = {k: v.cpu().numpy() for k, v in res.solved_tuples().items() if k not in ("own", "opp")}
    B["n_tuples"] = int(res.tuples()["pi"].shape[0])
    return B


def _run(nets, n_games, what, one_launch, k=K, n_sims=N_SIMS, **kw):
    """One call of a fresh engine: what(eng, k, n_sims) -> result, with whole games in one launch allowed or not."""
    m, eng = _engine(nets, n_games, **kw)
    was = os.environ.get("IAGO_PERSISTENT_GAMES")
    os.environ["IAGO_PERSISTENT_GAMES"] = "1" if one_launch else "0"
    try:
        res = what(eng, k, n_sims)
    finally:
        if was is None:
            del os.environ["IAGO_PERSISTENT_GAMES"]
        else:
            os.environ["IAGO_PERSISTENT_GAMES"] = was
    B = _snap(nets, m, eng, res)
    m.close()
    return B


def _play(eng, k, n_sims):
    return eng.play(n_sims, solve_empties=k)


def _stream(eng, k, n_sims):
    return eng.play_stream(n_sims, 640, solve_empties=k)


def _stream_2560(eng, k, n_sims):
    return eng.play_stream(n_sims, 2560, solve_empties=k)


def _match(eng, k, n_sims):
    colours = torch.where(torch.arange(eng.B) % 2 == 0, 1, 2).to(torch.int8)
    return eng.play_match(n_sims, mcts_colour=colours, solve_empties=k)


@pytest.fixture(scope="module")
def one(nets):
    return _run(nets, 256, _play, True)


@pytest.fixture(scope="module")
def loop(nets):
    return _run(nets, 256, _play, False)


@pytest.fixture(scope="module")
def plain(nets):
    return _run(nets, 256, _play, True, k=None)


@pytest.fixture(scope="module")
def split_one(nets):
    return _run(nets, 2048, _play, True)


@pytest.fixture(scope="module")
def split_loop(nets):
    return _run(nets, 2048, _play, False)


@pytest.fixture(scope="module")
def split4096_one(nets):
    return _run(nets, 4096, _play, True)


@pytest.fixture(scope="module")
def split4096_loop(nets):
    return _run(nets, 4096, _play, False)


@pytest.fixture(scope="module")
def split1100_one(nets):
    return _run(nets, 1100, _play, True, n_sims=60)


@pytest.fixture(scope="module")
def split1100_loop(nets):
    return _run(nets, 1100, _play, False, n_sims=60)


@pytest.fixture(scope="module")
def split_stream_one(nets):
    return _run(nets, 2048, _stream_2560, True)


@pytest.fixture(scope="module")
def split_stream_loop(nets):
    return _run(nets, 2048, _stream_2560, False)


@pytest.fixture(scope="module")
def stream_one(nets):
    return _run(nets, 256, _stream, True)


@pytest.fixture(scope="module")
def stream_loop(nets):
    return _run(nets, 256, _stream, False)


@pytest.fixture(scope="module")
def match(nets):
    # (whole games in one launch ALLOWED: a match with solve_empties must stay on the turn loop all the same)
    return _run(nets, 256, _match, True)


def _same_records(a, b):
    assert a["n_turns"] == b["n_turns"]
    for key in RECORDS:
        assert np.array_equal(a[key], b[key]), key


# ---------------------------------------------------------------- 1. the play-out kernel against the host reference
def test_play_endgame_against_host_reference(nets):
    ops = nets[1]
    own, opp = ref.late_positions(512, 71, 1, 10)
    n = len(own)
    games, cols = [], []
    for parity in (0, 1):
        for flag in (0, 1):
            for i in range(n):
                stones = 64 - ref.empties(own[i], opp[i])
                turn = 2 * (stones // 2) - 4 + parity      # (about where such a game stands; both parities)
                games.append((int(own[i]), int(opp[i]), turn, stones, flag, T))
    want = play_ref.play_out_many(games, workers=min(16, os.cpu_count() or 1))
    N = len(games)
    d_own = ops.bits_to_tensor([g[0] for g in games])
    d_opp = ops.bits_to_tensor([g[1] for g in games])
    d_turn = torch.tensor([g[2] for g in games], dtype=torch.int32, device="cuda")
    d_stones = torch.tensor([g[3] for g in games], dtype=torch.int32, device="cuda")
    d_flag = torch.tensor([g[4] for g in games], dtype=torch.uint8, device="cuda")
    parked = torch.ones(N, dtype=torch.uint8, device="cuda")
    parked[5::7] = 0                                        # games that are not parked are not touched
    in_own, in_opp, in_turn = d_own.clone(), d_opp.clone(), d_turn.clone()
    out = ops.play_endgame(d_own, d_opp, d_turn, d_stones, d_flag, parked, max_turns=T, max_empties=10, time_limit_ms=2000)
    ctl = out["ctl"].tolist()
    assert ctl[0] == 0 and ctl[2] == 0 and ctl[3] == 0, ctl
    finished, pk = out["finished"].cpu().numpy(), parked.cpu().numpy()
    assert np.array_equal(finished, pk)
    r_own, r_opp = ops.tensor_to_bits(out["own"]), ops.tensor_to_bits(out["opp"])
    r_valid, r_move, r_score = (out[k].cpu().numpy() for k in ("valid", "move", "score"))
    f_own, f_opp, f_turn = ops.tensor_to_bits(d_own), ops.tensor_to_bits(d_opp), d_turn.cpu().numpy()
    e_own, e_opp = np.zeros((T, N), np.uint64), np.zeros((T, N), np.uint64)
    e_valid, e_move, e_score = np.zeros((T, N), np.uint8), np.full((T, N), -1, np.int8), np.zeros((T, N), np.int8)
    n_pass = 0
    for g, w in enumerate(want):
        if not pk[g]:
            assert (int(f_own[g]), int(f_opp[g]), int(f_turn[g])) == games[g][:3]
            continue
        for t, a, b, valid, move, score in w["rows"]:
            e_own[t, g], e_opp[t, g], e_valid[t, g], e_move[t, g], e_score[t, g] = a, b, valid, move, score
            n_pass += valid == 0
        assert (int(f_own[g]), int(f_opp[g]), int(f_turn[g])) == (w["own"], w["opp"], w["n_turns"]), g
    for name, got, exp in (("own", r_own, e_own), ("opp", r_opp, e_opp), ("valid", r_valid, e_valid),
                           ("move", r_move, e_move), ("score", r_score, e_score)):
        assert np.array_equal(got, exp), name
    assert n_pass > 0 and len({w["n_turns"] % 2 for w in want}) == 1
    # every solved row is ops.solve_endgame's answer for its position
    rows = np.nonzero(r_valid.reshape(-1) == 3)[0]
    ex = ops.solve_endgame(ops.bits_to_tensor(r_own.reshape(-1)[rows]), ops.bits_to_tensor(r_opp.reshape(-1)[rows]),
                           max_empties=10, time_limit_ms=2000)
    assert np.array_equal(ex["score"].cpu().numpy(), r_score.reshape(-1)[rows])
    assert np.array_equal(ex["move"].cpu().numpy(), r_move.reshape(-1)[rows])
    assert len(rows) > 2000


# ---------------------------------------------------------------- 2. the two paths agree
def test_one_launch_equals_turn_loop(one, loop):
    assert one["launches"] == 2 and one["replayed"] == 0 and one["ctl3"] == 0
    assert loop["launches"] == loop["n_turns"] > 2
    _same_records(one, loop)
    assert one["sim"] == loop["sim"] and one["leaf_evals"] == loop["leaf_evals"]
    for key in one["solved_tuples"]:
        assert np.array_equal(one["solved_tuples"][key], loop["solved_tuples"][key]), key
    assert (one["valid"] == 3).sum() == one["n_solved_tuples"] > 256


def _split_engaged(B):
    """Whether the launch took the role split.  On the MI355X it must; elsewhere a runtime may give no CU-masked streams."""
    if not B["split"]:
        assert not torch.cuda.get_device_properties(0).gcnArchName.startswith("gfx950"), "the role split did not engage"
        pytest.skip("this runtime gives no CU-masked streams")


@pytest.mark.parametrize("size", ["", "4096", "1100"])
def test_role_split_equals_turn_loop(request, size):
    """2048 and 4096 games x 100 playouts, 1100 games x 60 (34 game workgroups of 32 games and one of 12: the games
    park by game id, past the last workgroup's slots)."""
    a, b = request.getfixturevalue("split%s_one" % size), request.getfixturevalue("split%s_loop" % size)
    _split_engaged(a)
    n_sims = 60 if size == "1100" else N_SIMS
    assert a["valid"].shape[1] == int(size or 2048)
    assert a["launches"] == 2 and a["replayed"] == 0 and a["ctl3"] == 0
    assert b["launches"] == b["n_turns"]
    _same_records(a, b)
    assert a["sim"] == b["sim"] == a["n_turns"] * n_sims
    assert a["leaf_evals"] == b["leaf_evals"] == (a["valid"] == 1).sum() * n_sims
    assert (a["valid"] == 3).sum() == a["n_solved_tuples"] > a["valid"].shape[1]


def test_split_stream_equals_batch_loop(split_stream_one, split_stream_loop):
    """2560 games through 2048 slots in one split launch + the play-out: games 2048 .. 2559 are claimed on the device
    and park by their id, not their slot.  Game G is game G of the batch loop (two batches through the turn loop)."""
    a, b = split_stream_one, split_stream_loop
    _split_engaged(a)
    assert a["launches"] == 2 and a["replayed"] == 0 and a["ctl3"] == 0
    assert b["launches"] == -(-2560 // 2048) and a["valid"].shape[1] == 2560     # (the batch loop counts its batches)
    _same_records(a, b)
    assert a["sim"] == b["sim"]
    assert (a["valid"][:, 2048:] == 3).sum() > 512


def test_stream_equals_batch_loop(stream_one, stream_loop):
    assert stream_one["launches"] == 2 and stream_one["replayed"] == 0 and stream_one["ctl3"] == 0
    assert stream_loop["launches"] == 3
    assert stream_one["valid"].shape[1] == 640
    _same_records(stream_one, stream_loop)
    assert stream_one["sim"] == stream_loop["sim"]


# ---------------------------------------------------------------- 3. the prefix is the plain game's
def _first_solved(B):
    v = B["valid"] == 3
    return np.where(v.any(axis=0), v.argmax(axis=0), B["valid"].shape[0])


def test_prefix_is_the_unsolved_game(one, plain):
    assert plain["launches"] == 1 and (plain["valid"] == 3).sum() == 0 and not plain["score"].any()
    first = _first_solved(one)
    assert (first < one["n_turns"]).sum() > 200
    for g in range(256):
        t = min(int(first[g]), plain["n_turns"])
        for key in ("own", "opp", "valid", "move", "pi"):
            assert np.array_equal(one[key][:t, g], plain[key][:t, g]), (g, key)


# ---------------------------------------------------------------- 4. exactness
def _check_exact(B, k):
    valid, own, opp = B["valid"], B["own"], B["opp"]
    n = 0
    for t, g in zip(*np.nonzero(valid == 3)):
        a, b = int(own[t, g]), int(opp[t, g])
        assert ref.empties(a, b) <= k
        assert (int(B["score"][t, g]), int(B["move"][t, g])) == orc.solve_endgame(a, b)[:2], (t, g)
        assert not B["pi"][t, g].any()
        n += 1
    for t, g in zip(*np.nonzero(valid == 1)):
        assert ref.empties(int(own[t, g]), int(opp[t, g])) > k, (t, g)
    assert not B["score"][valid != 3].any()
    return n


@pytest.mark.parametrize("name", ["one", "stream_one", "split_one", "split_stream_one"])
def test_solved_rows_are_the_c_references(request, name):
    B = request.getfixturevalue(name)
    if name.startswith("split"):
        _split_engaged(B)
    assert _check_exact(B, K) > B["valid"].shape[1]
    first = _first_solved(B)
    for g in np.nonzero(first < B["n_turns"])[0]:
        t = int(first[g])
        s = int(B["score"][t, g])
        z_mover = int(B["z"][g]) * (1 if t % 2 == 0 else -1)
        assert z_mover == (s > 0) - (s < 0), g
        # ... and the final disc difference is that score
        d = bin(int(B["f1"][g])).count("1") - bin(int(B["f2"][g])).count("1")
        assert d * (1 if t % 2 == 0 else -1) == s, g


# ---------------------------------------------------------------- 5. the match
def test_match_solves_pv_mcts_late_turns(match):
    B = match
    valid, own, opp, col = B["valid"], B["own"], B["opp"], B["mcts_colour"]
    # (the turn loop, although whole games in one launch were allowed: a launch per turn, and solved rows)
    assert B["launches"] == B["n_turns"] > 2 and set(col.tolist()) == {1, 2}
    assert _check_exact(B, K) > 100 and (valid == 3).sum() > 100
    n_policy_late = 0
    for t in range(B["n_turns"]):
        mover = 1 if t % 2 == 0 else 2
        for g in range(valid.shape[1]):
            late = ref.empties(int(own[t, g]), int(opp[t, g])) <= K
            if valid[t, g] == 3:
                assert col[g] == mover
            if valid[t, g] and col[g] != mover:
                assert valid[t, g] == 2
                n_policy_late += late
            if valid[t, g] == 2 and col[g] == mover:       # PV-MCTS without a search or a solve: the forced final move
                lm = ref.bit_legal(int(own[t, g]), int(opp[t, g]))
                assert lm & (lm - 1) == 0
            if valid[t, g] == 1:
                assert col[g] == mover and not late
    assert n_policy_late > 100
    first = _first_solved(B)
    for g in np.nonzero(first < B["n_turns"])[0]:
        t = int(first[g])
        d = bin(int(B["f1"][g])).count("1") - bin(int(B["f2"][g])).count("1")
        assert d * (1 if col[g] == 1 else -1) >= int(B["score"][t, g]), g
    assert B["tuples_valid"] == (valid == 1).sum() and B["n_solved_tuples"] == (valid == 3).sum()


# ---------------------------------------------------------------- 6. the counters
@pytest.mark.parametrize("name", ["one", "loop", "stream_one", "match"])
def test_counters(request, name):
    B = request.getfixturevalue(name)
    assert B["leaf_evals"] == (B["valid"] == 1).sum() * N_SIMS
    assert B["sim"] == B["n_turns"] * N_SIMS
    assert B["n_tuples"] == (B["valid"] == 1).sum()
