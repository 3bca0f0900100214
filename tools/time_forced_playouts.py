"""Times noised self-play with and without forced playouts and policy-target pruning
(SelfPlayEngine.play(root_noise=..., forced_playouts=k_256)), the shipped nets, the two settings interleaved batch by batch
in one process.

    python tools/time_forced_playouts.py [--games 1024] [--sims 100] [--alpha 77] [--eps 64] [--draws 256] [--k 512]
                                         [--batches 10] [--warmup 2]

Both settings run through the turn loop (root noise has no whole-game launch), so the ratio is the cost of the rule: the
forced selections in the search, what they do to the games' paths, and one launch of the pruning kernel per turn.  As in
tools/time_root_noise.py every setting meets the position table as the earlier batches of both settings left it, never
its own games: disjoint game ids (batch b: ids (2 b + j) x games for setting j), the order alternating.  There is no
threshold on the ratio: it is reported.  Prints one JSON line per setting and one with the ratio; the forced setting's
line also gives the share of the searched rows' visits that the pruning took out.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.time_playout_cap import make_engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--alpha", type=int, default=77)
    ap.add_argument("--eps", type=int, default=64)
    ap.add_argument("--draws", type=int, default=256)
    ap.add_argument("--k", type=int, default=512)
    ap.add_argument("--batches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    m, eng = make_engine(a.games, a.sims)
    noise = (a.alpha, a.eps, a.draws)
    settings = (("noised", None), ("forced", a.k))
    acc = {name: dict(walls=[], value=0, policy=0, hits=0, raw=0, pruned=0) for name, _ in settings}
    for batch in range(a.warmup + a.batches):
        order = list(enumerate(settings))
        order = order[batch % 2:] + order[:batch % 2]
        for j, (name, k) in order:
            m.game_id_base = (2 * batch + j) * a.games   # (other games every batch and in every setting)
            m.sim_counter = 0
            before = m._ps["totals"].clone()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = eng.play(a.sims, record=True, root_noise=noise, forced_playouts=k)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            if batch < a.warmup:
                continue
            d = (m._ps["totals"] - before).tolist()
            s = acc[name]
            s["walls"].append(wall)
            s["value"] += d[0]
            s["policy"] += d[1]
            s["hits"] += d[8]
            if res.pi_raw is not None:   # (after the clock)
                s["raw"] += int(res.pi_raw.sum().item())
                s["pruned"] += int(res.pi.sum().item())
    out = {}
    for name, k in settings:
        s, n = acc[name], a.batches * a.games
        out[name] = a.games / statistics.median(s["walls"])
        line = dict(what=name, root_noise=noise, forced_playouts=k, games=a.games, sims=a.sims, batches=a.batches,
                    split_cus=m.split_cus, games_per_s=out[name], games_per_s_all=n / sum(s["walls"]),
                    wall_min=min(s["walls"]), wall_max=max(s["walls"]), value_evals_per_game=s["value"] / n,
                    policy_evals_per_game=s["policy"] / n, table_hits_per_game=s["hits"] / n, replayed=eng.n_replayed)
        if s["raw"]:
            line["visits_pruned_share"] = 1.0 - s["pruned"] / s["raw"]
        print(json.dumps(line), flush=True)
    print(json.dumps(dict(what="ratios", forced_over_noised=out["forced"] / out["noised"])), flush=True)
    m.close()


if __name__ == "__main__":
    main()
