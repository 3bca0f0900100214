#!/usr/bin/env python3
"""The AlphaZero selection rule against the reference's (engine.BatchedMCTS(selection=)), the shipped nets and the same
constants on both sides.

    python tools/run_selection_arena.py [--games 1024] [--sims 100] [--explore-turns 8] [--seed 5] [--n-thr 15]
                                        [--c-puct 1.0] [--backup negamax] [--one-launch | --sequential]

Arena (engine.ArenaEngine): agent A selects by the AlphaZero rule (stored prior prob, U = c_puct P sqrt(N) / (1 + n)),
agent B by the reference's (prob + 0.1, 0.01 + n); both back up by --backup.  A plays colour 1 in the first half of the
games and colour 2 in the rest; the moves of the first --explore-turns turns are drawn from the visit counts so that the
games differ; A's rollouts draw under --seed, B's under --seed + 1.  --c-puct is A's alone: B keeps 1.0, the constant the
reference chose for its own denominator.
Prints one JSON line: alphazero's W / D / L against the reference rule overall and per colour, with scores (a draw counts
1/2) and 95 % Wilson intervals."""
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
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--explore-turns", type=int, default=8)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--n-thr", type=int, default=15)
    ap.add_argument("--c-puct", type=float, default=1.0)
    ap.add_argument("--backup", default="negamax")
    form = ap.add_mutually_exclusive_group()
    form.add_argument("--one-launch", dest="one_launch", action="store_true", default=None)
    form.add_argument("--sequential", dest="one_launch", action="store_false")
    args = ap.parse_args()
    from iago_amd import engine, network, ops
    from run_match import tally
    policy = network.SLPolicy().load_npz(os.path.join(GOLDEN, "sl_model.npz")).cuda().eval()
    value = network.Value().load_npz(os.path.join(GOLDEN, "value_model.npz")).cuda().eval()
    rollout = network.RolloutPolicy().load_npz(os.path.join(GOLDEN, "rollout_model.npz")).eval()
    rw = ops.RolloutWeights(*rollout.kernel_weights())
    B = args.games
    ms = [engine.BatchedMCTS(B, policy, value, rw, lmbda=0.5, c_puct=args.c_puct if rule == "alphazero" else 1.0,
                             n_thr=args.n_thr, seed=args.seed + k, persistent=True, backup=args.backup, selection=rule,
                             capacity=engine.suggest_capacity(args.sims, args.n_thr, moves=64))
          for k, rule in enumerate(("alphazero", "reference"))]
    arena = engine.ArenaEngine(*ms)
    r = arena.play(args.sims, record=False, explore_turns=args.explore_turns or None, one_launch=args.one_launch)
    z = r.z.to(torch.int32) * torch.where(r.a_colour == 1, 1, -1).to(torch.int32)
    c = r.a_colour
    out = dict(tool="run_selection_arena", games=B, n_sims=args.sims, explore_turns=args.explore_turns, n_thr=args.n_thr,
               seed=args.seed, backup=ms[0].backup, c_puct=[m.c_puct for m in ms], arena_launches=arena.n_arena_launches,
               gave_up=[int(m._ps["ctl"][3].item()) for m in ms], overflow=[int(m.tree.overflow.sum().item()) for m in ms],
               alphazero_vs_reference=dict(overall=tally(z), as_colour_1=tally(z[c == 1]), as_colour_2=tally(z[c == 2])))
    for m in ms:
        m.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
