#!/usr/bin/env python3
"""Times the fixed-depth alpha-beta opponent (ops.alphabeta_moves): ONE launch of --n midgame positions (seeded
uniform-random games cut at 20 to 40 empties) at depths 2 / 4 / 6 / 8, HIP events around the launch, the best of --reps
launches after one untimed warm-up.  Per depth: ms, the nodes visited, nodes/s of the launch, nodes/s per lane (a lane per
position: the launch's rate over n) and the rate of the lane with the most nodes, which the launch waits for.

    python tools/time_alphabeta.py [--n 1024] [--depths 2,4,6,8] [--reps 3] [--out profiles/alphabeta_bench.json]

Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def midgame_positions(n, seed, lo=20, hi=40):
    """n positions (own to move, with a legal move) of uniform-random games from the start (ops.random_moves), game g cut
    after a seeded number of turns so that lo..hi empties remain."""
    from iago_amd import ops
    rs = np.random.RandomState(seed)
    cut = torch.from_numpy(rs.randint(60 - hi, 60 - lo + 1, n)).cuda()      # turns played before the cut
    own = torch.full((n,), 0x0000000810000000, dtype=torch.int64, device="cuda")
    opp = torch.full((n,), 0x0000001008000000, dtype=torch.int64, device="cuda")
    for t in range(60 - lo):
        mv = ops.random_moves(own, opp, seed, 0, n, t)                      # (-1: the mover passes)
        o, p = ops.apply_moves(own.clone(), opp.clone(), mv)
        go = t < cut
        own, opp = torch.where(go, p, own), torch.where(go, o, opp)         # the stone, then the swap of sides
    e = 64 - _popcount(own | opp)
    ok = (ops.legal_moves(own, opp) != 0) & (e >= lo) & (e <= hi)
    return own[ok].contiguous(), opp[ok].contiguous()


def _popcount(x):
    cells = torch.arange(64, device=x.device)
    return ((x.reshape(-1, 1) >> cells) & 1).sum(dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--depths", default="2,4,6,8")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "alphabeta_bench.json"))
    args = ap.parse_args()
    from iago_amd import ops
    own, opp = midgame_positions(2 * args.n, args.seed)
    own, opp = own[:args.n].contiguous(), opp[:args.n].contiguous()
    n = own.numel()
    empties = 64 - _popcount(own | opp)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    rows = []
    for depth in (int(d) for d in args.depths.split(",")):
        ops.alphabeta_moves(own, opp, depth)                # warm-up (code object, allocator): not counted
        best, nodes = None, None
        for _ in range(args.reps):
            torch.cuda.synchronize()
            e0.record()
            r = ops.alphabeta_moves(own, opp, depth, check_result=False)
            e1.record()
            torch.cuda.synchronize()
            assert bool(r["done"].all()) and int(r["ctl"][0]) == 0
            ms = e0.elapsed_time(e1)
            if best is None or ms < best:
                best, nodes = ms, int(r["nodes"].sum().item())
        slowest = int(r["nodes"].max().item())
        # (a lane per position: the mean lane's rate, and the rate of the lane with the most nodes -- the launch waits for it)
        rows.append(dict(depth=depth, ms=round(best, 3), nodes=nodes, nodes_per_position=round(nodes / n, 1),
                         nodes_per_s=round(nodes / (best / 1e3)), nodes_per_s_per_lane=round(nodes / (best / 1e3) / n),
                         slowest_position_nodes=slowest, slowest_lane_nodes_per_s=round(slowest / (best / 1e3))))
    out = dict(tool="time_alphabeta", n=n, seed=args.seed, empties=[int(empties.min()), int(empties.max())],
               reps=args.reps, device=torch.cuda.get_device_name(0), depths=rows)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
