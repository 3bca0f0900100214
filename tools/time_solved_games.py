"""Times whole self-play games with the endgame played by the exact solver (SelfPlayEngine.play / play_stream with
solve_empties = None / 6 / 8 / 10, the same seeds) and records play_match scores at None and 8, with the shipped nets.

    python tools/time_solved_games.py [--games 1024] [--sims 100] [--batches 20] [--reps 3] [--match-games 1024]

Prints one JSON line per measurement: wall seconds per call (median of --reps after one warm-up call), turns, launches,
searched and solved rows, and for the matches PV-MCTS's score.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from iago_amd import engine, network, ops  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


def make_engine(n_games, n_sims, seed=7):
    policy = network.SLPolicy().load_npz(os.path.join(GOLDEN, "sl_model.npz")).cuda().eval()
    value = network.Value().load_npz(os.path.join(GOLDEN, "value_model.npz")).cuda().eval()
    value.split_f16 = True
    with open(os.path.join(GOLDEN, "simulate.json")) as f:
        g = json.load(f)
    m = engine.BatchedMCTS(n_games, policy, value, ops.RolloutWeights(g["shipped_w"], g["shipped_b"]), lmbda=0.5,
                           c_puct=1.0, n_thr=15, seed=seed, persistent=True,
                           capacity=engine.suggest_capacity(n_sims, 15, moves=64))
    m.warmup()
    return m, engine.SelfPlayEngine(m, max_turns=128)


def timed(m, call, reps):
    walls, res = [], None
    for rep in range(reps + 1):
        m.sim_counter, m.n_leaf_evals = 0, 0      # (the same seeds every call)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = call()
        torch.cuda.synchronize()
        if rep:
            walls.append(time.perf_counter() - t0)
    return res, walls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--match-games", type=int, default=1024)
    ap.add_argument("--ks", default="none,6,8,10")
    a = ap.parse_args()
    ks = [None if k == "none" else int(k) for k in a.ks.split(",")]
    m, eng = make_engine(a.games, a.sims)
    for name, call_of in (("play", lambda k: lambda: eng.play(a.sims, record=True, solve_empties=k)),
                          ("play_stream", lambda k: lambda: eng.play_stream(a.sims, a.batches * a.games, record=True,
                                                                            solve_empties=k))):
        for k in ks:
            res, walls = timed(m, call_of(k), a.reps if name == "play" else max(1, a.reps // 3))
            n = res.valid.shape[1]
            print(json.dumps(dict(what=name, solve_empties=k, games=n, sims=a.sims, wall_s=statistics.median(walls),
                                  walls=walls, games_per_s=n / statistics.median(walls), n_turns=res.n_turns,
                                  launches=res.launches, searched_rows=int((res.valid == 1).sum()),
                                  solved_rows=int((res.valid == 3).sum()), replayed=eng.n_replayed)), flush=True)
    m.close()
    if a.match_games > 0:
        m, eng = make_engine(a.match_games, a.sims)
        for k in (None, 8):
            m.sim_counter = 0
            t0 = time.perf_counter()
            res = eng.play_match(a.sims, mcts_colour=2, solve_empties=k)
            torch.cuda.synchronize()
            print(json.dumps(dict(what="play_match", solve_empties=k, games=a.match_games, sims=a.sims,
                                  wall_s=time.perf_counter() - t0, launches=res.launches, score=res.score(),
                                  solved_rows=int((res.valid == 3).sum()))), flush=True)
        m.close()


if __name__ == "__main__":
    main()
