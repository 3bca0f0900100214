#!/usr/bin/env python3
"""Times the fixed-depth alpha-beta opponent (ops.alphabeta_moves): ONE launch of --n midgame positions (seeded
uniform-random games cut at 20 to 40 empties) at depths 2 / 4 / 6 / 8, HIP events around the launch, the best of --reps
launches after one untimed warm-up.  Per depth: ms, the nodes visited, nodes/s of the launch, nodes/s per lane (a lane per
position: the launch's rate over n) and the rate of the lane with the most nodes, which the launch waits for.

    python tools/time_alphabeta.py [--n 1024] [--depths 2,4,6,8] [--reps 3] [--out profiles/alphabeta_bench.json]

--split 0,1,2 (default 0: the rows above) times the root split beside the unsplit launch in one process, on the same
positions, for every n of --n (a list: the first n of the positions): per (n, depth, split) ms, the jobs, their room
(play_match's: n x engine.ALPHABETA_JOBS_PER_ROOT, no readback inside the timed call) and the total nodes -- the split's
jobs share no bound, so it visits more nodes than the unsplit search and wins only by spreading them.  A split that is
not below the depth is left out.  --out is then profiles/alphabeta_split_bench.json:

    python tools/time_alphabeta.py --split 0,1,2 --n 1,512,1024 --depths 4,6,8

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


def time_splits(args, all_own, all_opp, ns, splits):
    """The rows of --split: every (n, depth, split) with split < depth, the best of --reps launches after a warm-up."""
    from iago_amd import engine, ops
    out_path = args.out or os.path.join(ROOT, "profiles", "alphabeta_split_bench.json")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    rows = []
    for n in ns:
        own, opp = all_own[:n].contiguous(), all_opp[:n].contiguous()
        assert own.numel() == n
        for depth in (int(d) for d in args.depths.split(",")):
            want = None
            for split in splits:
                if split >= depth:
                    continue
                room = n * engine.ALPHABETA_JOBS_PER_ROOT[split] if split else None
                kw = dict(split=split, job_capacity=room) if split else {}
                ops.alphabeta_moves(own, opp, depth, **kw)      # warm-up, and checked: nothing refused, no overflow
                best = None
                for _ in range(args.reps):
                    torch.cuda.synchronize()
                    e0.record()
                    r = ops.alphabeta_moves(own, opp, depth, check_result=False, **kw)
                    e1.record()
                    torch.cuda.synchronize()
                    ms = e0.elapsed_time(e1)
                    best = ms if best is None else min(best, ms)
                assert bool(r["done"].all()) and int(r["ctl"][0]) == 0
                got = (r["score"].clone(), r["move"].clone())
                if want is None:
                    want = got
                assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])   # every split: the same answers
                nodes = int(r["nodes"].sum().item())
                row = dict(n=n, depth=depth, split=split, ms=round(best, 3), nodes=nodes,
                           nodes_per_s=round(nodes / (best / 1e3)), slowest_position_nodes=int(r["nodes"].max().item()))
                if split:
                    jobs = ops.alphabeta_job_count(r["ctl"].tolist())
                    row.update(jobs=jobs, job_capacity=room, most_jobs_of_a_root=int(r["job_count"].max().item()),
                               slowest_job_nodes=int(r["job_nodes"][:jobs].max().item()))
                rows.append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
    out = dict(tool="time_alphabeta", seed=args.seed, reps=args.reps, device=torch.cuda.get_device_name(0), rows=rows)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="1024")
    ap.add_argument("--split", default="0")
    ap.add_argument("--depths", default="2,4,6,8")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from iago_amd import ops
    ns, splits = [int(v) for v in args.n.split(",")], [int(v) for v in args.split.split(",")]
    own, opp = midgame_positions(2 * max(ns), args.seed)
    if splits != [0] or len(ns) > 1:
        return time_splits(args, own, opp, ns, splits)
    args.out = args.out or os.path.join(ROOT, "profiles", "alphabeta_bench.json")
    own, opp = own[:ns[0]].contiguous(), opp[:ns[0]].contiguous()
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
