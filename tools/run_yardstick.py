#!/usr/bin/env python3
"""The shipped nets (tests/golden/sl_model.npz, value_model.npz, rollout_model.npz) against the fixed-depth alpha-beta
opponent, the one strength figure here that owes nothing to the nets: SelfPlayEngine.play_match(opponent=AlphaBeta(d),
opening_turns=8, paired=True) -- --games games per cell, every random opening played once with PV-MCTS as colour 1 and
once as colour 2 -- at every playout count of --sims, under both backup rules, against every depth of --depths.

    python tools/run_yardstick.py [--games 1024] [--sims 100,400] [--depths 1,2,4,6] [--backups reference,negamax]
                                  [--selections reference] [--c-pucts 1.0] [--append]
                                  [--opening-turns 8] [--seed 5] [--split 0] [--out profiles/alphabeta_yardstick.json]

--selections: the selection rules (engine.selection_arg: "reference", "alphazero"), --c-pucts: the exploration constants;
every combination with --backups and --sims is a row of cells.  --append: the cells are added to those --out already
holds (same games, opening turns and seed, or refused) instead of replacing them.  --split: the opponent's root split
(engine.AlphaBeta(depth, split): the same moves, launched over more lanes), at a depth that has no room for it the
largest split below the depth; a cell records the split it ran with and the turns whose jobs overflowed their room.

Per cell: PV-MCTS's wins / draws / losses, its score (a draw counting 1/2) with the 95 % Wilson interval, overall and per
colour, the turns of the longest game and the wall time of the match (one untimed warm-up match per engine before its
cells).  Prints one JSON line and writes it to --out."""
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
    ap.add_argument("--sims", default="100,400")
    ap.add_argument("--depths", default="1,2,4,6")
    ap.add_argument("--backups", default="reference,negamax")
    ap.add_argument("--selections", default="reference")
    ap.add_argument("--c-pucts", default="1.0")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--opening-turns", type=int, default=8)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--split", type=int, default=0, choices=(0, 1, 2))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "alphabeta_yardstick.json"))
    args = ap.parse_args()
    from iago_amd import engine, network, ops
    policy = network.SLPolicy().load_npz(os.path.join(GOLDEN, "sl_model.npz")).cuda().eval()
    value = network.Value().load_npz(os.path.join(GOLDEN, "value_model.npz")).cuda().eval()
    rollout = network.RolloutPolicy().load_npz(os.path.join(GOLDEN, "rollout_model.npz")).eval()
    B = args.games
    cells = []
    if args.append and os.path.exists(args.out):
        with open(args.out) as f:
            old = json.loads(f.readline())
        if (old["games"], old["opening_turns"], old["seed"]) != (B, args.opening_turns, args.seed):
            raise SystemExit("--append: %s holds cells of other games, opening turns or seed" % args.out)
        cells = old["cells"]

    def save():
        line = json.dumps(dict(tool="run_yardstick", games=B, opening_turns=args.opening_turns, paired=True, seed=args.seed,
                               device=torch.cuda.get_device_name(0), cells=cells))
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
        return line

    line = None
    rows = [(backup, selection, c_puct, sims) for backup in args.backups.split(",")
            for selection in args.selections.split(",") for c_puct in (float(c) for c in args.c_pucts.split(","))
            for sims in (int(s) for s in args.sims.split(","))]
    for backup, selection, c_puct, sims in rows:
        m = engine.BatchedMCTS(B, policy, value, ops.RolloutWeights(*rollout.kernel_weights()), lmbda=0.5, c_puct=c_puct,
                               n_thr=15, seed=args.seed, persistent=True, backup=backup, selection=selection,
                               capacity=engine.suggest_capacity(sims, 15, moves=64))
        eng = engine.SelfPlayEngine(m)
        kw = dict(opening_turns=args.opening_turns, paired=True, record=False)
        eng.play_match(sims, opponent=engine.AlphaBeta(1), **kw)   # warm-up (allocator, code objects): not counted
        for depth in (int(d) for d in args.depths.split(",")):
            m.sim_counter = 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            split = min(args.split, depth - 1)
            r = eng.play_match(sims, opponent=engine.AlphaBeta(depth, split=split), **kw)
            torch.cuda.synchronize()
            s = time.perf_counter() - t0
            z = r.z.to(torch.int32) * torch.where(r.mcts_colour == 1, 1, -1).to(torch.int32)
            c = r.mcts_colour
            cells.append(dict(backup=backup, selection=selection, c_puct=c_puct, n_sims=sims, depth=depth, s=round(s, 2),
                              turns=r.n_turns, split=split, split_overflows=r.split_overflows,
                              mcts=dict(overall=tally(z), as_colour_1=tally(z[c == 1]), as_colour_2=tally(z[c == 2]))))
            print(json.dumps(cells[-1]), file=sys.stderr, flush=True)
        m.close()
        line = save()   # (after every row: a run that is cut short keeps the rows it finished)
    print(line)


if __name__ == "__main__":
    main()
