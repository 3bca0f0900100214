#!/usr/bin/env python3
"""PV-MCTS against the SL policy it is built on -- the reference's `game.py --auto` -- with the shipped checkpoints
(tests/golden/sl_model.npz, value_model.npz, rollout_model.npz), through SelfPlayEngine.play_match.

    python tools/run_match.py [--games 1024] [--batches 2] [--sims 100] [--seed 5]

K = --batches batches of B = --games games (batch k: game_id_base k x B, every batch from the same sim_counter), PV-MCTS
playing colour 1 in half of every batch's games (the odd ones) and colour 2 (the reference's setting) in the other half.
Prints one JSON line: games/s over HIP events around the batches (the first, untimed warm-up batch excluded), the
launches they took, and PV-MCTS's score per colour and overall -- wins, draws, losses, the score (a draw counting 1/2) and
its 95 % Wilson interval."""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def wilson(score, n, z=1.96):
    """95 % Wilson score interval of a proportion (draws counted as half a win)."""
    if n == 0:
        return [float("nan"), float("nan")]
    p = score / n
    d = 1.0 + z * z / n
    c = (p + z * z / (2 * n)) / d
    h = z * math.sqrt(p * (1 - p) / n + z * z / (4 * n * n)) / d
    return [round(c - h, 4), round(c + h, 4)]


def tally(z_mcts):
    w, d, l = (int(v) for v in torch.stack([(z_mcts > 0).sum(), (z_mcts == 0).sum(), (z_mcts < 0).sum()]).tolist())
    n = w + d + l
    s = w + 0.5 * d
    return dict(wins=w, draws=d, losses=l, n=n, score=round(s / n, 4) if n else None, wilson95=wilson(s, n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--selfplay", action="store_true", help="also time play() (self-play) on the same batches")
    args = ap.parse_args()
    from iago_amd import engine, network, ops
    policy = network.SLPolicy().load_npz(os.path.join(GOLDEN, "sl_model.npz")).cuda().eval()
    value = network.Value().load_npz(os.path.join(GOLDEN, "value_model.npz")).cuda().eval()
    rollout = network.RolloutPolicy().load_npz(os.path.join(GOLDEN, "rollout_model.npz")).eval()
    B = args.games
    m = engine.BatchedMCTS(B, policy, value, ops.RolloutWeights(*rollout.kernel_weights()), lmbda=0.5, c_puct=1.0,
                           n_thr=15, seed=args.seed, persistent=True,
                           capacity=engine.suggest_capacity(args.sims, 15, moves=64))
    eng = engine.SelfPlayEngine(m)
    colours = torch.full((B,), 2, dtype=torch.int64, device="cuda")
    colours[1::2] = 1
    eng.play_match(args.sims, mcts_colour=colours, record=False)      # warm-up (allocator, code objects): not counted
    m.sim_counter = 0
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    zs, cs, launches, turns = [], [], 0, 0
    for k in range(args.batches):
        m.game_id_base, m.sim_counter = k * B, 0
        r = eng.play_match(args.sims, mcts_colour=colours, record=False)
        zs.append(r.z.to(torch.int32) * torch.where(r.mcts_colour == 1, 1, -1).to(torch.int32))
        cs.append(r.mcts_colour)
        launches += r.launches
        turns = max(turns, r.n_turns)
    e1.record()
    torch.cuda.synchronize()
    s = e0.elapsed_time(e1) / 1e3
    z, c = torch.cat(zs), torch.cat(cs)
    games = args.batches * B
    out = dict(tool="run_match", games=games, batch=B, batches=args.batches, n_sims=args.sims, seed=args.seed,
               s=round(s, 3), games_per_s=round(games / s, 2), launches=launches, longest_game_turns=turns,
               replayed=getattr(eng, "n_replayed", 0), split=m._split is not None,
               mcts=dict(overall=tally(z), as_colour_1=tally(z[c == 1]), as_colour_2=tally(z[c == 2])))
    if args.selfplay:                  # the same batches as PV-MCTS self-play: the games/s a match is compared with
        m.sim_counter = 0
        eng.play(args.sims, record=False)
        torch.cuda.synchronize()
        e0.record()
        for k in range(args.batches):
            m.game_id_base, m.sim_counter = k * B, 0
            eng.play(args.sims, record=False)
        e1.record()
        torch.cuda.synchronize()
        sp = e0.elapsed_time(e1) / 1e3
        out["selfplay_games_per_s"] = round(games / sp, 2)
        out["match_over_selfplay"] = round(sp / s, 4)
    m.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
