#!/usr/bin/env python3
"""Two PV-MCTS agents against each other (engine.ArenaEngine), each with its own Chainer npz checkpoints.

    python tools/run_arena.py POLICY_A.npz VALUE_A.npz POLICY_B.npz VALUE_B.npz [--sims-a 100] [--sims-b 100]
                              [--lmbda-a 0.5] [--lmbda-b 0.5] [--games 256] [--batches 1] [--seed 5] [--n-thr 15]
                              [--one-launch | --sequential] [--backup-a reference] [--backup-b reference]
                              [--selection-a reference] [--selection-b reference]

K = --batches batches of B = --games games; A plays colour 1 in the first half of every batch's games and colour 2 in
the rest; the rollouts are the shipped RolloutPolicy's on both sides, A draws them under --seed and B under --seed + 1.
--backup-a / --backup-b: each agent's backup rule (engine.backup_arg: "reference" or "negamax").
--selection-a / --selection-b: each agent's selection rule (engine.selection_arg: "reference" or "alphazero").
Prints one JSON line: A's score (wins, draws, losses, the score with a draw counting 1/2, its 95 % Wilson interval), per
colour and overall, and games/s over HIP events around the batches (one untimed warm-up batch first)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("policy_a")
    ap.add_argument("value_a")
    ap.add_argument("policy_b")
    ap.add_argument("value_b")
    ap.add_argument("--sims-a", type=int, default=100)
    ap.add_argument("--sims-b", type=int, default=100)
    ap.add_argument("--lmbda-a", type=float, default=0.5)
    ap.add_argument("--lmbda-b", type=float, default=0.5)
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--batches", type=int, default=1)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--n-thr", type=int, default=15)
    ap.add_argument("--backup-a", default="reference")
    ap.add_argument("--backup-b", default="reference")
    ap.add_argument("--selection-a", default="reference")
    ap.add_argument("--selection-b", default="reference")
    form = ap.add_mutually_exclusive_group()
    form.add_argument("--one-launch", dest="one_launch", action="store_true", default=None)
    form.add_argument("--sequential", dest="one_launch", action="store_false")
    args = ap.parse_args()
    from iago_amd import engine, network, ops
    from run_match import tally
    rollout = network.RolloutPolicy().load_npz(os.path.join(GOLDEN, "rollout_model.npz")).eval()
    rw = ops.RolloutWeights(*rollout.kernel_weights())
    B = args.games
    ms = []
    for k, (p, v, lm, n, bk, sel) in enumerate(((args.policy_a, args.value_a, args.lmbda_a, args.sims_a, args.backup_a,
                                                 args.selection_a),
                                                (args.policy_b, args.value_b, args.lmbda_b, args.sims_b, args.backup_b,
                                                 args.selection_b))):
        policy = network.SLPolicy().load_npz(p).cuda().eval()
        value = network.Value().load_npz(v).cuda().eval()
        ms.append(engine.BatchedMCTS(B, policy, value, rw, lmbda=lm, c_puct=1.0, n_thr=args.n_thr, seed=args.seed + k,
                                     persistent=True, capacity=engine.suggest_capacity(n, args.n_thr), backup=bk,
                                     selection=sel))
    arena = engine.ArenaEngine(*ms)
    sims = (args.sims_a, args.sims_b)
    arena.play(sims, record=False, one_launch=args.one_launch)      # warm-up: not counted
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    zs, cs, launches = [], [], 0
    for k in range(args.batches):
        for m in ms:
            m.game_id_base, m.sim_counter = k * B, 0
        r = arena.play(sims, record=False, one_launch=args.one_launch)
        zs.append(r.z.to(torch.int32) * torch.where(r.a_colour == 1, 1, -1).to(torch.int32))
        cs.append(r.a_colour)
        launches += r.launches
    e1.record()
    torch.cuda.synchronize()
    s = e0.elapsed_time(e1) / 1e3
    z, c = torch.cat(zs), torch.cat(cs)
    games = args.batches * B
    print(json.dumps(dict(tool="run_arena", games=games, batch=B, batches=args.batches, n_sims=list(sims),
                          lmbda=[args.lmbda_a, args.lmbda_b], backup=[m.backup for m in ms],
                          selection=[m.selection for m in ms], n_thr=args.n_thr,
                          seed=args.seed, s=round(s, 3),
                          games_per_s=round(games / s, 2), launches=launches, arena_launches=arena.n_arena_launches,
                          a=dict(overall=tally(z), as_colour_1=tally(z[c == 1]), as_colour_2=tally(z[c == 2])))))
    for m in ms:
        m.close()


if __name__ == "__main__":
    main()
