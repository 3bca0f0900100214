#!/usr/bin/env python3
"""The Gumbel root search against the plain search at small budgets, on the alpha-beta yardstick: the shipped nets
(tests/golden/sl_model.npz, value_model.npz, rollout_model.npz) play SelfPlayEngine.play_match(opponent=AlphaBeta(d,
split=2), opening_turns=8, paired=True) -- --games games per cell, every random opening once with PV-MCTS as colour 1 and
once as colour 2 -- under the negamax backup and the AlphaZero selection at n_thr = 1, at every playout count of --sims,
with gumbel=(m, c_scale_256) and without, against every depth of --depths.  One run per cell.

    python tools/run_gumbel_yardstick.py [--games 1024] [--sims 16,32,64] [--depths 2,4] [--m 16] [--c-scale 256]
                                         [--opening-turns 8] [--seed 5] [--out profiles/gumbel_yardstick.json]

Per cell: PV-MCTS's wins / draws / losses, its score (a draw counting 1/2) with the 95 % Wilson interval and its
half-width, the turns of the longest game and the wall time of the match (one untimed warm-up match per engine before its
cells).  Nothing is asserted about the outcome.  Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def main():
    from run_match import tally
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--sims", default="16,32,64")
    ap.add_argument("--depths", default="2,4")
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--c-scale", type=int, default=256)
    ap.add_argument("--opening-turns", type=int, default=8)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gumbel_yardstick.json"))
    args = ap.parse_args()
    from iago_amd import engine, network, ops
    policy = network.SLPolicy().load_npz(os.path.join(GOLDEN, "sl_model.npz")).cuda().eval()
    value = network.Value().load_npz(os.path.join(GOLDEN, "value_model.npz")).cuda().eval()
    rollout = network.RolloutPolicy().load_npz(os.path.join(GOLDEN, "rollout_model.npz")).eval()
    B = args.games
    cells = []

    def save():
        line = json.dumps(dict(tool="run_gumbel_yardstick", games=B, opening_turns=args.opening_turns, paired=True,
                               seed=args.seed, backup="negamax", selection="alphazero", n_thr=1, split=2,
                               device=torch.cuda.get_device_name(0), cells=cells))
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
        return line

    line = None
    for sims in (int(s) for s in args.sims.split(",")):
        m = engine.BatchedMCTS(B, policy, value, ops.RolloutWeights(*rollout.kernel_weights()), lmbda=0.5, c_puct=1.0, n_thr=1,
                               seed=args.seed, persistent=True, backup="negamax", selection="alphazero",
                               capacity=engine.suggest_capacity(sims, 1, moves=64))
        eng = engine.SelfPlayEngine(m)
        kw = dict(opening_turns=args.opening_turns, paired=True, record=False)
        for gumbel in ((args.m, args.c_scale), None):
            eng.play_match(sims, opponent=engine.AlphaBeta(1), gumbel=gumbel, **kw)   # warm-up: not counted
            for depth in (int(d) for d in args.depths.split(",")):
                m.sim_counter = 0
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                split = min(2, depth - 1)
                r = eng.play_match(sims, opponent=engine.AlphaBeta(depth, split=split), gumbel=gumbel, **kw)
                torch.cuda.synchronize()
                s = time.perf_counter() - t0
                z = r.z.to(torch.int32) * torch.where(r.mcts_colour == 1, 1, -1).to(torch.int32)
                t = tally(z)
                lo, hi = t["wilson95"]
                cells.append(dict(gumbel=list(gumbel) if gumbel else None, n_sims=sims, depth=depth, s=round(s, 2),
                                  turns=r.n_turns, split=split, split_overflows=r.split_overflows, mcts=t,
                                  half_width=round((hi - lo) / 2, 4)))
                print(json.dumps(cells[-1]), file=sys.stderr, flush=True)
        m.close()
        line = save()   # (after every budget: a run that is cut short keeps the cells it finished)
    print(line)


if __name__ == "__main__":
    main()
