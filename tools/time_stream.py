#!/usr/bin/env python3
"""The self-play stream against the batch loop, at the headline's size (1024 slots, random-init nets as bench.py's).

    python tools/time_stream.py [--slots 1024] [--batches 20] [--sims 100,400]

For each playout count, K = --batches batches' worth of games three ways -- the SAME games each way (batch k with
game_id_base k x slots, every batch from the same sim_counter: play_stream's batch loop):
  (a) K play() calls, the position table zeroed before each (as bench.py's headline step);
  (b) K play() calls, the table kept (a user's loop);
  (c) ONE play_stream(n_sims, K x slots), the table zeroed once before it.
Per way: games/s and leaf-evals/s over HIP events around the way (synchronised), value evaluations and table hits per
game (totals[0], totals[8]), the net workgroups' busy fraction (walking / (waiting + walking): totals[5], totals[4]).
(c) against (b) is the stream alone; against (a) the stream plus the table reaching across batches.  Prints one
JSON line."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def engine_for(n_slots, n_sims):
    from iago_amd import engine, network, ops
    from tests.conftest import load_json
    g = load_json("simulate.json")
    torch.manual_seed(0)
    policy = network.SLPolicy().cuda().eval()
    value = network.Value().cuda().eval()
    m = engine.BatchedMCTS(n_slots, policy, value, ops.RolloutWeights(g["shipped_w"], g["shipped_b"]), lmbda=0.5,
                           c_puct=1.0, n_thr=15, seed=7, persistent=True,
                           capacity=engine.suggest_capacity(n_sims, 15, moves=64))
    return engine, m


def run_way(engine, m, way, n_sims, k_batches):
    eng = engine.SelfPlayEngine(m)
    n = m.n_games
    s0 = m.sim_counter
    m._ps["totals"].zero_()
    leaf0 = m.n_leaf_evals
    if m._vtable is not None:
        m._vtable.zero_()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    zs = []
    if way == "c":
        r = eng.play_stream(n_sims, k_batches * n)
        launches = r.launches
        zs.append(r.z)
    else:
        for k in range(k_batches):
            if way == "a" and k and m._vtable is not None:
                m._vtable.zero_()
            m.game_id_base, m.sim_counter = k * n, s0
            zs.append(eng.play(n_sims).z)
        m.game_id_base = 0
        launches = k_batches
    e1.record()
    torch.cuda.synchronize()
    s = e0.elapsed_time(e1) / 1e3
    m.sim_counter = s0
    tot = m._ps["totals"].tolist()
    games = k_batches * n
    leaf = m.n_leaf_evals - leaf0
    busy = tot[5] / max(tot[4] + tot[5], 1)
    return dict(s=round(s, 3), games_per_s=round(games / s, 1), leaf_evals_per_s=round(leaf / s), launches=launches,
                value_evals_per_game=round(tot[0] / games, 1), table_hits_per_game=round(tot[8] / games, 1),
                net_busy=round(busy, 4)), torch.cat(zs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=1024)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--sims", default="100,400")
    args = ap.parse_args()
    out = dict(tool="time_stream", slots=args.slots, batches=args.batches, results={})
    for n_sims in [int(x) for x in args.sims.split(",")]:
        engine, m = engine_for(args.slots, n_sims)
        engine.SelfPlayEngine(m, max_turns=4).play(16)          # (allocator, code objects)
        m.sim_counter = 0
        res, z = {}, {}
        for way in ("a", "b", "c"):
            res[way], z[way] = run_way(engine, m, way, n_sims, args.batches)
        res["c_over_b"] = round(res["c"]["games_per_s"] / res["b"]["games_per_s"], 4)
        res["c_over_a"] = round(res["c"]["games_per_s"] / res["a"]["games_per_s"], 4)
        res["same_games"] = bool(torch.equal(z["a"], z["c"]) and torch.equal(z["b"], z["c"]))
        out["results"][str(n_sims)] = res
        m.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
