#!/usr/bin/env python3
"""Speed of the exact endgame solver (ops.solve_endgame / engine.solve_endgame, include/iago_hip_serving.h).

    python tools/time_endgame.py [--batch 4096] [--batch-empties 8,10,12,14,16] [--single-empties 12,14,16,18]
                                 [--splits 0,1,2,3,4] [--reps 5] [--limit-ms 20000] [--moves best,all] [--out FILE]
                                 [--device-splits 0,1,2] [--split-batches 1024,4096]

Positions: seeded SLPolicy-vs-SLPolicy games (rl_self_play.play_batch, the shipped sl_model.npz), the recorded
positions of colour 1 at exactly E empties.  Prints one JSON line per measurement:
  * batch: `--batch` positions at E empties in one launch, both modes -- positions/s and nodes/s over HIP events;
  * single: one position at E empties through engine.solve_endgame(split_depth=k) -- the median wall time of `--reps`
    positions (host split and minimax included), its nodes.
  * --moves best,all: the batch measurement also through ops.solve_endgame_moves with each of the named root rules,
    on the same positions (kind "batch_moves": its time and nodes, and both as ratios to the plain launch's).
  * --device-splits 0,1,2: the device-side root split (ops.solve_endgame(split=), iago_solve_endgame_split) in place
    of the two batch measurements above: for every size of --split-batches, every E of --batch-empties, both modes, the
    plain call and moves="all", one launch per named split on the same positions (kind "batch_split": seconds over HIP
    events with the count-only launch and its readback included, nodes, jobs, the slowest job's nodes, and same_answer
    against the row's split 0 -- score, move and under "all" best and move_score); and next to every "single" row one
    position through ops.solve_endgame(split=k), k > 0 (kind "single_split": the median wall time of the same `--reps`
    positions).
A launch that gives up at --limit-ms is reported as such.  --out FILE: the lines also go to FILE, as one JSON list."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def positions_at(policy, empties, n, seed):
    """n positions with exactly `empties` empties from seeded policy-vs-policy games (own = colour 1 to move)."""
    from iago_amd import ops, rl_self_play
    own, opp, k = [], [], 0
    while len(own) < n:
        r = rl_self_play.play_batch(policy, policy, 1024, seed=seed + k, game_id_base=1024 * k)
        k += 1
        o, p = ops.tensor_to_bits(r["own"]), ops.tensor_to_bits(r["opp"])
        for g in range(o.shape[1]):
            for t in range(o.shape[0]):
                if o[t, g] | p[t, g] and 64 - bin(int(o[t, g] | p[t, g])).count("1") == empties:
                    own.append(o[t, g])
                    opp.append(p[t, g])
                    break
    return np.array(own[:n], np.uint64), np.array(opp[:n], np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--batch-empties", default="8,10,12,14,16")
    ap.add_argument("--single-empties", default="12,14,16,18")
    ap.add_argument("--splits", default="0,1,2,3,4")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit-ms", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--moves", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--device-splits", default="")
    ap.add_argument("--split-batches", default="")
    args = ap.parse_args()
    from iago_amd import _lib, engine, network, ops
    policy = network.SLPolicy().load_npz(os.path.join(GOLDEN, "sl_model.npz")).cuda().eval()
    ints = lambda s: [int(x) for x in s.split(",") if x]   # noqa: E731
    rules = [x for x in args.moves.split(",") if x]
    lines = []

    def emit(**row):
        lines.append(dict(tool="time_endgame", **row))
        print(json.dumps(lines[-1]), flush=True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    w = positions_at(policy, 6, 64, args.seed)
    ops.solve_endgame(ops.bits_to_tensor(w[0]), ops.bits_to_tensor(w[1]))   # warm-up: code object, allocator
    for rule in rules:
        ops.solve_endgame_moves(ops.bits_to_tensor(w[0]), ops.bits_to_tensor(w[1]), moves=rule)
    device_splits = ints(args.device_splits)

    def timed(fn):
        torch.cuda.synchronize()
        e0.record()
        r = fn()
        e1.record()
        torch.cuda.synchronize()
        return r, e0.elapsed_time(e1) / 1e3

    def split_columns(r, base, keys):
        """What a batch_split / single_split row says about one launch r; base: the same positions at split 0."""
        jobs = ops.alphabeta_job_count(r["ctl"].tolist()) if "job_count" in r else 0
        return dict(solved=int(r["solved"].sum().item()), gave_up=bool(r["ctl"][0].item()),
                    nodes=int(r["nodes"].sum().item()), max_nodes=int(r["nodes"].max().item()), jobs=jobs,
                    max_job_nodes=int(r["job_nodes"].max().item()) if jobs else 0,
                    same_answer=all(bool(torch.equal(r[k], base[k])) for k in keys))

    if device_splits:
        for k in device_splits:   # warm-up of the split's kernels
            ops.solve_endgame_moves(ops.bits_to_tensor(w[0]), ops.bits_to_tensor(w[1]), moves="all", split=k)
        sizes = ints(args.split_batches) or [args.batch]
        for E in ints(args.batch_empties):
            o, p = positions_at(policy, E, max(sizes), args.seed + 100 * E)
            for n in sizes:
                to, tp = ops.bits_to_tensor(o[:n]), ops.bits_to_tensor(p[:n])
                for mode in ("exact", "wld"):
                    for rule in ("", "all"):
                        kw = dict(mode=mode, max_empties=E, time_limit_ms=args.limit_ms, check_result=False)
                        call = (lambda k: ops.solve_endgame_moves(to, tp, moves="all", split=k, **kw)) if rule else \
                            (lambda k: ops.solve_endgame(to, tp, split=k, **kw))
                        keys = ("score", "move", "solved") + (("best", "move_score") if rule else ())
                        base, _ = timed(lambda: call(0))
                        for k in device_splits:
                            r, s = timed(lambda: call(k))
                            emit(kind="batch_split", empties=E, mode=mode, moves=rule, n=n, split=k, s=round(s, 4),
                                 **split_columns(r, base, keys))
    for E in ([] if device_splits else ints(args.batch_empties)):
        o, p = positions_at(policy, E, args.batch, args.seed + 100 * E)
        to, tp = ops.bits_to_tensor(o), ops.bits_to_tensor(p)
        for mode in ("exact", "wld"):
            torch.cuda.synchronize()
            e0.record()
            r = ops.solve_endgame(to, tp, mode=mode, max_empties=E, time_limit_ms=args.limit_ms, check_result=False)
            e1.record()
            torch.cuda.synchronize()
            s = e0.elapsed_time(e1) / 1e3
            nodes = int(r["nodes"].sum().item())
            solved = int(r["solved"].sum().item())
            emit(kind="batch", empties=E, mode=mode, n=len(o), solved=solved, gave_up=bool(r["ctl"][0].item()),
                 s=round(s, 4), positions_per_s=round(solved / s, 1), nodes=nodes, mnodes_per_s=round(nodes / s / 1e6, 2),
                 max_nodes=int(r["nodes"].max().item()))
            for rule in rules:
                torch.cuda.synchronize()
                e0.record()
                q = ops.solve_endgame_moves(to, tp, mode=mode, moves=rule, max_empties=E, time_limit_ms=args.limit_ms,
                                            check_result=False)
                e1.record()
                torch.cuda.synchronize()
                sq = e0.elapsed_time(e1) / 1e3
                nq = int(q["nodes"].sum().item())
                emit(kind="batch_moves", moves=rule, empties=E, mode=mode, n=len(o), solved=int(q["solved"].sum().item()),
                     gave_up=bool(q["ctl"][0].item()), s=round(sq, 4), nodes=nq, mnodes_per_s=round(nq / sq / 1e6, 2),
                     time_ratio=round(sq / s, 3), node_ratio=round(nq / nodes, 3),
                     same_answer=bool((q["score"] == r["score"]).all().item() and (q["move"] == r["move"]).all().item()))
    for E in ints(args.single_empties):
        o, p = positions_at(policy, E, args.reps, args.seed + 1000 + E)
        for k in ints(args.splits):
            times, nodes, gave_up = [], [], False
            for i in range(len(o)):
                to, tp = ops.bits_to_tensor(o[i:i + 1]), ops.bits_to_tensor(p[i:i + 1])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                try:
                    r = engine.solve_endgame(to, tp, split_depth=k, time_limit_ms=args.limit_ms)
                    torch.cuda.synchronize()
                except _lib.IagoError:
                    gave_up = True
                    break
                times.append(time.perf_counter() - t0)
                nodes.append(int(r["nodes"][0].item()))
            emit(kind="single", empties=E, split_depth=k, reps=len(times), gave_up=gave_up,
                 median_ms=round(1e3 * float(np.median(times)), 2) if times else None,
                 max_ms=round(1e3 * max(times), 2) if times else None,
                 median_nodes=int(np.median(nodes)) if nodes else None)
        kw = dict(max_empties=E, time_limit_ms=args.limit_ms, check_result=False)
        bases = [ops.solve_endgame(ops.bits_to_tensor(o[i:i + 1]), ops.bits_to_tensor(p[i:i + 1]), **kw)
                 for i in range(len(o) if any(device_splits) else 0)]
        for k in [k for k in device_splits if k > 0]:
            times, cols = [], []
            for i, base in enumerate(bases):
                to, tp = ops.bits_to_tensor(o[i:i + 1]), ops.bits_to_tensor(p[i:i + 1])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = ops.solve_endgame(to, tp, split=k, **kw)
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
                cols.append(split_columns(r, base, ("score", "move", "solved")))
            emit(kind="single_split", empties=E, split=k, reps=len(times), gave_up=any(c["gave_up"] for c in cols),
                 median_ms=round(1e3 * float(np.median(times)), 2), max_ms=round(1e3 * max(times), 2),
                 median_nodes=int(np.median([c["nodes"] for c in cols])), median_jobs=int(np.median([c["jobs"] for c in cols])),
                 max_job_nodes=max(c["max_job_nodes"] for c in cols), same_answer=all(c["same_answer"] for c in cols))
    if args.out:
        with open(args.out, "w") as f:
            f.write("[\n" + ",\n".join(json.dumps(x, sort_keys=True) for x in lines) + "\n]\n")


if __name__ == "__main__":
    main()
