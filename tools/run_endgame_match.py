#!/usr/bin/env python3
"""SLPolicy against PV-MCTS through the front end (game.Game(auto=True), the reference's `game.py --auto`: the policy
plays colour 1, MCTS colour 2) with the shipped checkpoints, with and without the exact endgame solver
(MCTS(solve_empties=k)), on the same seeds.

    python tools/run_endgame_match.py [--games 256] [--sims 100] [--solve-empties 12] [--seed 5]

Game g of both runs draws the policy's moves from numpy RandomState(seed + g) and searches with MCTS seed seed + g.
Prints one JSON line per run: PV-MCTS's wins, draws, losses, score (a draw counting 1/2) with its 95 % Wilson interval,
moves played by the solver, seconds."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--solve-empties", type=int, default=12)
    ap.add_argument("--seed", type=int, default=5)
    args = ap.parse_args()
    from run_match import wilson
    from iago_amd import game as game_mod
    from iago_amd import network, ops
    from iago_amd.MCTS import MCTS
    policy = network.SLPolicy().load_npz(os.path.join(GOLDEN, "sl_model.npz")).cuda().eval()
    value = network.Value().load_npz(os.path.join(GOLDEN, "value_model.npz")).cuda().eval()
    rollout = network.RolloutPolicy().load_npz(os.path.join(GOLDEN, "rollout_model.npz")).eval()
    rw = ops.RolloutWeights(*rollout.kernel_weights())
    for k in (None, args.solve_empties):
        w = d = l = solved = 0
        t0 = time.time()
        for g in range(args.games):
            m = MCTS(policy_net=policy, value_net=value, rollout_weights=rw, n_sims=args.sims, seed=args.seed + g,
                     capacity=65536, solve_empties=k)
            game = game_mod.Game(True, model=policy, mcts=m, date="match", out=lambda *_: None,
                                 choice=np.random.RandomState(args.seed + g).choice)
            game_mod.play(game, True)
            me, op = int(np.sum(game.state == 2)), int(np.sum(game.state == 1))
            w, d, l = w + (me > op), d + (me == op), l + (me < op)
            solved += m.n_solved
        n = w + d + l
        s = w + 0.5 * d
        print(json.dumps(dict(tool="run_endgame_match", solve_empties=k, n_sims=args.sims, games=n, seed=args.seed,
                              mcts=dict(wins=w, draws=d, losses=l, score=round(s / n, 4), wilson95=wilson(s, n)),
                              solver_moves=solved, s=round(time.time() - t0, 1))), flush=True)


if __name__ == "__main__":
    main()
