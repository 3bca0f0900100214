"""Every optimal move and every move's value from the exact solver, on the device: ops.solve_endgame_moves against the
restatement of its root rules (tests/endgame_moves_ref.py) and, at 11 - 12 empties, against the C reference alone; its
refusals; ops.play_endgame(best=True); SelfPlayEngine.play / play_stream(solved_targets=True) on both paths;
engine.endgame_errors.  Positions of at most 12 empties: milliseconds of device time."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from iago_amd import _lib, engine, ops
from oracle import oracle as orc
from tests.bench_batch_util import make_nets
from tests.conftest import load_json

from . import endgame_moves_ref as mr
from . import endgame_ref as er
from . import lane_search_ref as ls

pytestmark = pytest.mark.gpu

NO_MOVE = _lib.ENDGAME_NO_MOVE


def _np(r):
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}


def _u64(x):
    return int(x) & 0xFFFFFFFFFFFFFFFF


@pytest.fixture(scope="module")
def roots():
    """The 64 late positions of 2 to 10 empties, then the hand-made roots."""
    own, opp = er.late_positions(64, 29, 2, 10)
    own, opp = [int(a) for a in own], [int(b) for b in opp]
    for _, a, b in mr.hand_made():
        own.append(a)
        opp.append(b)
    return own, opp


@pytest.fixture(scope="module")
def want(roots):
    """(wld, rule) -> [(score, move, nodes, best, scores)] of the restatement, computed once."""
    own, opp = roots
    return {(wld, rule): [mr.solve_moves(a, b, wld, rule) for a, b in zip(own, opp)]
            for wld in (False, True) for rule in (mr.BEST, mr.ALL)}


def _row(scores):
    row = [NO_MOVE] * 64
    for m, v in (scores or {}).items():
        row[m] = v
    return row


# ---------------------------------------------------------------- against the restatement
@pytest.mark.parametrize("mode", ["exact", "wld"])
@pytest.mark.parametrize("moves", ["best", "all"])
@pytest.mark.parametrize("n", [64, 1, 63, 65])
def test_against_the_restatement(roots, want, mode, moves, n):
    own, opp = roots
    N = len(own)
    # (launches of exactly n from the 69: the hand-made roots first, but for 64, which ends with them, and 1: a late one)
    idx = list(range(N - 64, N)) if n == 64 else [2] if n == 1 else [(64 + i) % N for i in range(n)]
    d_own, d_opp = ops.bits_to_tensor([own[i] for i in idx]), ops.bits_to_tensor([opp[i] for i in idx])
    r = _np(ops.solve_endgame_moves(d_own, d_opp, mode=mode, moves=moves, max_empties=10))
    plain = _np(ops.solve_endgame(d_own, d_opp, mode=mode, max_empties=10))
    assert r["solved"].all() and r["ctl"][0] == 0 and r["ctl"][2] == 0 and r["ctl"][3] == 0
    assert ("move_score" in r) == (moves == "all")
    w = [want[mode == "wld", moves][i] for i in idx]
    assert r["score"].tolist() == [x[0] for x in w] == plain["score"].tolist()
    assert r["move"].tolist() == [x[1] for x in w] == plain["move"].tolist()
    assert r["nodes"].tolist() == [x[2] for x in w]
    assert [_u64(b) for b in r["best"]] == [x[3] for x in w]
    legal = [er.bit_legal(own[i], opp[i]) for i in idx]
    kinds = set()
    for j, (x, lm) in enumerate(zip(w, legal)):
        kinds.add(min(x[1], 0))
        if x[1] < 0:           # a pass root, a finished game: the empty set
            assert x[3] == 0 and (lm == 0)
        else:
            assert x[1] == ls._lowest(x[3]) and x[3] & ~lm == 0
    assert n == 1 or kinds == {0, -1, -2}
    if moves == "all":
        assert r["move_score"].shape == (len(idx), 64) and r["move_score"].dtype == np.int8
        assert r["move_score"].tolist() == [_row(x[4]) for x in w]
        for j, lm in enumerate(legal):
            on = [a for a in range(64) if r["move_score"][j, a] != NO_MOVE]
            assert on == ([a for a in range(64) if lm >> a & 1] if w[j][1] >= 0 else [])


# ---------------------------------------------------------------- against the C oracle alone, 11 - 12 empties
@pytest.mark.parametrize("mode", ["exact", "wld"])
def test_deep_rows_against_the_c_reference(mode):
    fx = load_json("endgame_deep.json")
    rows = [r for e in (11, 12) for r in [r for r in fx["rows"] if r["empties"] == e and r[mode]][:4]]
    assert len(rows) == 8 and {r["empties"] for r in rows} == {11, 12}
    own, opp = [r["own"] for r in rows], [r["opp"] for r in rows]
    d_own, d_opp = ops.bits_to_tensor(own), ops.bits_to_tensor(opp)
    vals = [orc.root_values(a, b, wld=mode == "wld") for a, b in zip(own, opp)]
    out = {mv: _np(ops.solve_endgame_moves(d_own, d_opp, mode=mode, moves=mv, max_empties=12, time_limit_ms=20000))
           for mv in ("best", "all")}
    for j, (r, v) in enumerate(zip(rows, vals)):
        top = max(v.values()) if v else None
        for mv in ("best", "all"):
            o = out[mv]
            assert o["solved"][j] and [int(o["score"][j]), int(o["move"][j])] == r[mode][:2]
            if v:
                assert int(o["score"][j]) == top
                assert _u64(o["best"][j]) == sum(1 << m for m, x in v.items() if x == top)
            else:
                assert o["best"][j] == 0
        assert out["all"]["move_score"][j].tolist() == _row(v)
        assert out["best"]["nodes"][j] <= out["all"]["nodes"][j]


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("moves", ["best", "all"])
def test_device_side_refusals(roots, want, moves):
    own, opp = roots
    e = [er.empties(a, b) for a, b in zip(own[:64], opp[:64])]
    big = max(range(64), key=lambda i: e[i])
    small = min(range(64), key=lambda i: e[i] if er.bit_legal(own[i], opp[i]) else 99)
    assert e[big] > 6 >= e[small]
    o = [own[small], own[big], own[small] | 1 | 2, own[small]]
    p = [opp[small], opp[big], opp[small] | 1, opp[small]]    # (row 2: own & opp != 0)
    with pytest.raises(_lib.IagoError) as err:
        ops.solve_endgame_moves(ops.bits_to_tensor(o), ops.bits_to_tensor(p), moves=moves, max_empties=6)
    assert "iago_solve_endgame_moves: 2 positions refused" in str(err.value)
    r = _np(err.value.result)
    assert r["solved"].tolist() == [1, 0, 0, 1] and r["ctl"][2] == 2 and r["ctl"][0] == 0 and r["ctl"][3] == 0
    assert r["best"][1] == 0 and r["best"][2] == 0
    w = want[False, moves][small]
    for j in (0, 3):
        assert (int(r["score"][j]), int(r["move"][j]), int(r["nodes"][j]), _u64(r["best"][j])) == w[:4]
    if moves == "all":
        assert (r["move_score"][1] == NO_MOVE).all() and (r["move_score"][2] == NO_MOVE).all()
        assert r["move_score"][0].tolist() == _row(w[4])


def test_host_side_refusals():
    dev = "cuda"
    n = 2
    t = dict(own=torch.zeros(n, dtype=torch.int64, device=dev), opp=torch.zeros(n, dtype=torch.int64, device=dev),
             score=torch.zeros(n, dtype=torch.int8, device=dev), move=torch.zeros(n, dtype=torch.int8, device=dev),
             nodes=torch.zeros(n, dtype=torch.int64, device=dev), solved=torch.full((n,), 7, dtype=torch.uint8, device=dev),
             best=torch.zeros(n, dtype=torch.int64, device=dev), ctl=torch.full((4,), 7, dtype=torch.int32, device=dev),
             move_score=torch.zeros((n, 64), dtype=torch.int8, device=dev))
    L = _lib.lib()

    def args(**kw):
        a = _lib.EndgameMovesArgs()
        for k, v in t.items():
            if k != "move_score":
                setattr(a, k, v.data_ptr())
        a.n, a.mode, a.moves, a.max_empties, a.time_limit_ms = n, 0, 0, 8, 1000
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(a, what):
        assert L.iago_solve_endgame_moves(C.byref(a), None) == _lib.IAGO_ERR_INVALID
        msg = L.iago_last_error().decode()
        assert msg.startswith("iago_solve_endgame_moves: ") and what in msg, msg

    assert L.iago_solve_endgame_moves(None, None) == _lib.IAGO_ERR_INVALID
    for k in ("own", "opp", "score", "move", "nodes", "solved", "best", "ctl"):
        refused(args(**{k: None}), "null pointer")
    refused(args(n=-1), "negative n")
    for bad in (-1, 2):
        refused(args(mode=bad), "mode must be")
        refused(args(moves=bad), "moves must be")
    refused(args(move_score=t["move_score"].data_ptr()), "must be NULL under IAGO_ENDGAME_MOVES_BEST")
    refused(args(moves=_lib.ENDGAME_MOVES_ALL), "required under IAGO_ENDGAME_MOVES_ALL")
    for bad in (-1, 21):
        refused(args(max_empties=bad), "max_empties")
    for bad in (0, _lib.ENDGAME_MAX_TIME_MS + 1):
        refused(args(time_limit_ms=bad), "time_limit_ms")
    for i in range(4):
        a = args()
        a.reserved[i] = 1
        refused(a, "reserved fields must be 0")
    torch.cuda.synchronize()
    # nothing was launched or cleared
    assert t["solved"].tolist() == [7, 7] and t["ctl"].tolist() == [7] * 4
    with pytest.raises(ValueError):
        ops.solve_endgame_moves(t["own"], t["opp"], moves="every")
    with pytest.raises(ValueError):
        ops.solve_endgame_moves(t["own"], t["opp"], mode="sign")
    # the play-out's own refusals: iago_play_endgame's, and a missing rec_best
    m = _lib.PlayEndgameMovesArgs()
    assert L.iago_play_endgame_moves(None, None) == _lib.IAGO_ERR_INVALID
    rec = dict(own=torch.zeros((4, n), dtype=torch.int64, device=dev), valid=torch.zeros((4, n), dtype=torch.uint8, device=dev),
               move=torch.zeros((4, n), dtype=torch.int8, device=dev))
    p = m.play
    p.own, p.opp, p.turn = t["own"].data_ptr(), t["opp"].data_ptr(), torch.zeros(n, dtype=torch.int32, device=dev).data_ptr()
    keep = [torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)]
    p.turn, p.stones = keep[0].data_ptr(), keep[0].data_ptr()
    p.pass_flg, p.parked, p.finished = keep[1].data_ptr(), keep[1].data_ptr(), t["solved"].data_ptr()
    p.n, p.stride, p.max_turns, p.max_empties, p.time_limit_ms = n, n, 4, 8, 1000
    p.rec_own, p.rec_opp = rec["own"].data_ptr(), rec["own"].data_ptr()
    p.rec_valid, p.rec_move, p.rec_score, p.ctl = (rec["valid"].data_ptr(), rec["move"].data_ptr(), rec["move"].data_ptr(),
                                                   t["ctl"].data_ptr())

    def play_refused(what):
        assert L.iago_play_endgame_moves(C.byref(m), None) == _lib.IAGO_ERR_INVALID
        msg = L.iago_last_error().decode()
        assert msg.startswith("iago_play_endgame_moves: ") and what in msg, msg

    play_refused("null pointer")                      # rec_best
    m.rec_best = rec["own"].data_ptr()
    m.reserved[2] = 1
    play_refused("reserved fields must be 0")
    m.reserved[2] = 0
    p.reserved0 = 1
    play_refused("reserved fields must be 0")
    p.reserved0 = 0
    p.stride = n - 1
    play_refused("stride")
    p.stride, p.max_empties = n, 21
    play_refused("max_empties")
    torch.cuda.synchronize()
    assert t["solved"].tolist() == [7, 7] and t["ctl"].tolist() == [7] * 4


# ---------------------------------------------------------------- the play-out
def test_play_endgame_best_record():
    """8 games parked at 8 empties: every row of the best record is the restatement's set for that turn's position,
    every other record is ops.play_endgame's without the keyword."""
    own, opp = er.late_positions(8, 31, 8, 8)
    n, T = 8, 128

    def launch(**kw):
        o, p = ops.bits_to_tensor([int(a) for a in own]), ops.bits_to_tensor([int(b) for b in opp])
        turn = torch.full((n,), 52, dtype=torch.int32, device="cuda")
        out = ops.play_endgame(o, p, turn, torch.full((n,), 56, dtype=torch.int32, device="cuda"),
                               torch.zeros(n, dtype=torch.uint8, device="cuda"), max_turns=T, max_empties=8, **kw)
        out = dict(out, final_own=o, final_opp=p, turn=turn)
        return _np(out)

    a, b = launch(), launch(best=True)
    assert "best" not in a and b["best"].shape == (T, n) and b["best"].dtype == np.int64
    for k in a:
        if k != "ctl":
            assert np.array_equal(a[k], b[k]), k
    assert b["finished"].all() and b["ctl"][0] == 0 and b["ctl"][2] == 0 and b["ctl"][3] == 0
    solved = ties = 0
    for t in range(T):
        for g in range(n):
            if b["valid"][t, g] == 3:
                w = mr.solve_moves(_u64(b["own"][t, g]), _u64(b["opp"][t, g]), False, mr.BEST)
                assert (int(b["score"][t, g]), int(b["move"][t, g]), _u64(b["best"][t, g])) == (w[0], w[1], w[3]), (t, g)
                solved += 1
                ties += bin(w[3]).count("1") >= 2
            else:
                assert b["valid"][t, g] == 0 and b["best"][t, g] == 0
    assert solved >= 8 * 6 and ties >= 1
    # records given by the caller: the best record is required with the keyword
    with pytest.raises(KeyError):
        rec = {k: torch.from_numpy(a[k]).cuda() for k in ("own", "opp", "valid", "move", "score")}
        launch(best=True, records=rec)


# ---------------------------------------------------------------- the engine
N_THR, SEED, K, N_SIMS, T = 15, 7, 6, 20, 128
RECORDS = ("own", "opp", "valid", "move", "pi", "score", "z", "final_p1", "final_p2")


@pytest.fixture(scope="module")
def nets():
    policy, value = make_nets()
    g = load_json("simulate.json")
    return policy, value, ops.RolloutWeights(g["shipped_w"], g["shipped_b"])


def _games(nets, one_launch, stream=0, **kw):
    policy, value, shipped = nets
    m = engine.BatchedMCTS(16, policy, value, shipped, lmbda=0.5, c_puct=1.0, n_thr=N_THR, seed=SEED, persistent=True,
                           capacity=engine.suggest_capacity(N_SIMS, N_THR, moves=64))
    m.warmup()
    eng = engine.SelfPlayEngine(m, max_turns=T)
    was = os.environ.get("IAGO_PERSISTENT_GAMES")
    os.environ["IAGO_PERSISTENT_GAMES"] = "1" if one_launch else "0"
    try:
        res = eng.play_stream(N_SIMS, stream, solve_empties=K, **kw) if stream else eng.play(N_SIMS, solve_empties=K, **kw)
    finally:
        if was is None:
            del os.environ["IAGO_PERSISTENT_GAMES"]
        else:
            os.environ["IAGO_PERSISTENT_GAMES"] = was
    torch.cuda.synchronize()
    snap = {k: getattr(res, k).cpu().numpy() for k in RECORDS}
    snap["best"] = None if res.best is None else res.best.cpu().numpy()
    snap.update(res=res, launches=res.launches, n_turns=res.n_turns, replayed=eng.n_replayed)
    m.close()
    return snap


@pytest.fixture(scope="module")
def games(nets):
    return dict(one=_games(nets, True, solved_targets=True), loop=_games(nets, False, solved_targets=True),
                off_one=_games(nets, True), off_loop=_games(nets, False))


def _same(a, b, keys=RECORDS):
    assert a["n_turns"] == b["n_turns"]
    for k in keys:
        assert np.array_equal(a[k], b[k]), k


def test_engine_paths_record_the_same_targets(games):
    one, loop = games["one"], games["loop"]
    assert one["launches"] == 2 and one["replayed"] == 0 and loop["launches"] == loop["n_turns"] > 2
    _same(one, loop, RECORDS + ("best",))
    assert one["best"].shape == one["valid"].shape and one["best"].dtype == np.int64
    assert (one["valid"] == 3).sum() >= 16 * 4


def test_engine_without_the_flag_is_todays(games):
    for path in ("one", "loop"):
        off, on = games["off_" + path], games[path]
        _same(off, on)
        assert off["best"] is None and off["res"].best is None
        assert sorted(off["res"].solved_tuples()) == ["colour", "game", "move", "opp", "own", "score", "turn", "z"]
        assert off["launches"] == on["launches"]
    with pytest.raises(ValueError):
        engine._play_rules(N_SIMS, solved_targets=True)          # needs solve_empties
    with pytest.raises(ValueError):
        engine._play_rules(N_SIMS, solve_empties=6, solved_targets=1)
    assert engine._play_rules(N_SIMS, solve_empties=6) == engine.PlayRules(6, 0, None)


def test_engine_targets(games):
    s = games["one"]
    valid, best = s["valid"], s["best"]
    assert not best[valid != 3].any() and best[valid == 3].all()
    tup = {k: v.cpu().numpy() for k, v in s["res"].solved_tuples().items()}
    assert sorted(tup) == ["best", "colour", "game", "move", "opp", "own", "pi", "score", "turn", "z"]
    rows = int((valid == 3).sum())
    assert tup["pi"].shape == (rows, 64) and tup["pi"].dtype == np.int32 and set(np.unique(tup["pi"])) <= {0, 1}
    ties = 0
    for i in range(rows):
        b = _u64(tup["best"][i])
        assert tup["pi"][i].sum() == bin(b).count("1") >= 1
        assert [a for a in range(64) if tup["pi"][i, a]] == [a for a in range(64) if b >> a & 1]
        assert int(tup["move"][i]) == ls._lowest(b)
        w = mr.solve_moves(_u64(tup["own"][i]), _u64(tup["opp"][i]), False, mr.BEST)
        assert (int(tup["score"][i]), int(tup["move"][i]), b) == (w[0], w[1], w[3])
        ties += bin(b).count("1") >= 2
    assert ties >= 1


def test_the_trainer_and_the_window_take_the_rows(nets, games):
    from iago_amd import network
    from iago_amd.replay import ReplayWindow
    from iago_amd.train_rl import ReinforceTrainer
    tup = games["one"]["res"].solved_tuples()
    rows = int(tup["own"].numel())
    w = ReplayWindow(rows + 4, seed=1)
    assert w.add(tup) == rows
    model = network.SLPolicy()
    model.load_state_dict(nets[0].state_dict())
    tr = ReinforceTrainer(model, pool_dir=None, N=2, seed=1)
    out = tr.step_from_tuples(tup, target="visits")
    assert out["n_tuples"] == rows and np.isfinite(out["loss"])


def test_stream_records_the_targets(nets):
    """32 games through 16 slots: the one launch + play-out against the batch loop."""
    a, b = _games(nets, True, stream=32, solved_targets=True), _games(nets, False, stream=32, solved_targets=True)
    assert a["launches"] == 2 and a["replayed"] == 0 and b["launches"] == 2 and a["valid"].shape[1] == 32
    _same(a, b, RECORDS + ("best",))
    assert not a["best"][a["valid"] != 3].any() and a["best"][a["valid"] == 3].all()
    assert (a["valid"][:, 16:] == 3).sum() >= 16 * 4


# ---------------------------------------------------------------- endgame_errors
def test_endgame_errors(roots, want):
    own, opp = roots
    w = want[False, mr.ALL]
    keep = [i for i in range(len(own)) if w[i][1] >= 0]
    d_own, d_opp = ops.bits_to_tensor([own[i] for i in keep]), ops.bits_to_tensor([opp[i] for i in keep])
    # the solver's own move: no loss
    best = torch.tensor([w[i][1] for i in keep], dtype=torch.int8, device="cuda")
    r = engine.endgame_errors(d_own, d_opp, best, max_empties=10)
    assert r["rows"] == len(keep) and r["skipped"] == 0 and r["mean_loss"] == 0 and r["optimal_rate"] == 1
    assert r["blunder_rate"] == 0 and not r["loss"].any() and r["optimal"].all() and not r["blunder"].any()
    # every position's worst move: max - min, and the signs
    worst = [min(w[i][4], key=lambda m: (w[i][4][m], m)) for i in keep]
    r = engine.endgame_errors(d_own, d_opp, torch.tensor(worst, dtype=torch.int64, device="cuda"), max_empties=10)
    loss = [max(w[i][4].values()) - min(w[i][4].values()) for i in keep]
    sign = lambda v: (v > 0) - (v < 0)
    blunder = [sign(max(w[i][4].values())) != sign(min(w[i][4].values())) for i in keep]
    assert r["loss"].tolist() == loss and r["optimal"].tolist() == [x == 0 for x in loss]
    assert r["blunder"].tolist() == blunder and 0 < sum(blunder) < len(keep)
    assert r["mean_loss"] == pytest.approx(sum(loss) / len(keep)) and r["blunder_rate"] == pytest.approx(sum(blunder) / len(keep))
    assert r["optimal_rate"] == pytest.approx(sum(x == 0 for x in loss) / len(keep)) and (r["loss"] >= 0).all()
    assert r["score"].tolist() == [w[i][0] for i in keep] and r["index"].tolist() == list(range(len(keep)))
    # wld: outcomes given away
    ww = want[True, mr.ALL]
    r = engine.endgame_errors(d_own, d_opp, torch.tensor(worst, dtype=torch.int64, device="cuda"), max_empties=10, mode="wld")
    assert r["loss"].tolist() == [ww[i][0] - ww[i][4][m] for i, m in zip(keep, worst)]
    # skipped rows: passes / no turn (move < 0) and positions above max_empties, counted
    every = torch.tensor([w[i][1] for i in range(len(own))], dtype=torch.int8, device="cuda")
    r = engine.endgame_errors(ops.bits_to_tensor(own), ops.bits_to_tensor(opp), every, max_empties=6)
    kept = [i for i in range(len(own)) if w[i][1] >= 0 and er.empties(own[i], opp[i]) <= 6]
    assert r["index"].tolist() == kept and r["rows"] == len(kept) and r["skipped"] == len(own) - len(kept) > 3
    assert r["optimal"].all()
    # nothing kept
    r = engine.endgame_errors(d_own[:2], d_opp[:2], torch.tensor([-1, -1], dtype=torch.int8, device="cuda"))
    assert r["rows"] == 0 and r["skipped"] == 2 and np.isnan(r["mean_loss"])
    # an illegal move names its row
    bad = best.clone()
    i = 5
    bad[i] = next(a for a in range(64) if not er.bit_legal(own[keep[i]], opp[keep[i]]) >> a & 1)
    with pytest.raises(ValueError, match="row 5: move %d is not a legal move" % int(bad[i])):
        engine.endgame_errors(d_own, d_opp, bad, max_empties=10)
