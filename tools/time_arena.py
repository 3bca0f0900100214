#!/usr/bin/env python3
"""Whole arena rounds (engine.ArenaEngine: two PV-MCTS agents, each with its own module pair loaded from the shipped
checkpoints) timed in three forms, interleaved round by round on one device:
  (a) one launch per turn (iago_mcts_search_arena), (b) sequential (mcts_a.search, then mcts_b.search), and, for scale,
  (c) SelfPlayEngine._play_turns self-play of the same size on agent A's engine.

    python tools/time_arena.py [--games 1024] [--sims 100] [--rounds 6] [--seed 5]

Per form: games/s of every timed round (HIP events around the round; one untimed warm-up round per form first), their
median and spread (max - min over the median), and per agent the net workgroups' busy share of the form's timed rounds
(walking / (waiting + walking) ticks, totals[5] / (totals[4] + totals[5])).  One JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--seed", type=int, default=5)
    args = ap.parse_args()
    from iago_amd import engine, network, ops
    rollout = network.RolloutPolicy().load_npz(os.path.join(GOLDEN, "rollout_model.npz")).eval()
    rw = ops.RolloutWeights(*rollout.kernel_weights())
    B = args.games
    ms = []
    for k in range(2):   # (two module pairs: two weight sets in memory, as two rounds' nets are)
        policy = network.SLPolicy().load_npz(os.path.join(GOLDEN, "sl_model.npz")).cuda().eval()
        value = network.Value().load_npz(os.path.join(GOLDEN, "value_model.npz")).cuda().eval()
        ms.append(engine.BatchedMCTS(B, policy, value, rw, lmbda=0.5, c_puct=1.0, n_thr=15, seed=args.seed + k,
                                     game_id_base=k * B, persistent=True, capacity=engine.suggest_capacity(args.sims, 15)))
    arena = engine.ArenaEngine(*ms)
    sp = engine.SelfPlayEngine(ms[0])

    def selfplay():
        ms[0].tree.reset()
        return sp._play_turns([engine._Side(ms[0], args.sims)], *sp._start_boards(B), False, engine.SelfPlayResult(),
                              engine.NO_RULES)

    forms = [("one_launch", lambda: arena.play(args.sims, record=False, one_launch=True)),
             ("sequential", lambda: arena.play(args.sims, record=False, one_launch=False)),
             ("selfplay_turn_loop", selfplay)]
    rate = {name: [] for name, _ in forms}
    ticks = {name: [[0, 0], [0, 0]] for name, _ in forms}
    launches = {}
    for r in range(args.rounds + 1):              # (round 0: the warm-up of every form)
        for name, run in forms:
            for m in ms:
                m.sim_counter = 0
            before = [m._ps["totals"][4:6].clone() for m in ms]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            res = run()
            e1.record()
            torch.cuda.synchronize()
            if r == 0:
                continue
            rate[name].append(B / (e0.elapsed_time(e1) / 1e3))
            launches[name] = res.launches
            for k, m in enumerate(ms):
                d = (m._ps["totals"][4:6] - before[k]).tolist()
                ticks[name][k][0] += int(d[0])
                ticks[name][k][1] += int(d[1])
    out = dict(tool="time_arena", games=B, n_sims=args.sims, rounds=args.rounds, seed=args.seed,
               arena_net_workgroups=arena.net_workgroups, arena_launches=arena.n_arena_launches)
    for name, _ in forms:
        med = statistics.median(rate[name])
        out[name] = dict(games_per_s=[round(v, 2) for v in rate[name]], median=round(med, 2),
                         spread=round((max(rate[name]) - min(rate[name])) / med, 4), launches_per_round=launches[name],
                         net_busy_share={w: (round(t[1] / (t[0] + t[1]), 4) if t[0] + t[1] else None)
                                         for w, t in zip(("a", "b"), ticks[name])})
    a, b = out["one_launch"], out["sequential"]
    out["one_launch_over_sequential"] = round(a["median"] / b["median"], 4)
    # the rule of the default form: (a) only if it beats (b) by more than the spread of (b)'s own rounds
    out["one_launch_is_faster"] = bool(a["median"] > b["median"] * (1.0 + b["spread"]))
    for m in ms:
        m.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
