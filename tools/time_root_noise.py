"""Times whole self-play games with and without root noise (SelfPlayEngine.play(root_noise=(alpha_256, eps_256[, draws]))),
the shipped nets, the settings interleaved batch by batch in one process.

    python tools/time_root_noise.py [--games 1024] [--sims 100] [--alpha 77] [--eps 64] [--draws 256] [--batches 10]
                                    [--warmup 2]

Games with root noise run through the turn loop, plain games in one launch, so three settings are timed: plain (one
launch), plain through the turn loop (IAGO_PERSISTENT_GAMES=0: what the noise's path costs without the noise) and noised.
As in tools/time_playout_cap.py every setting meets the position table as the earlier batches of all settings left it,
never its own games: disjoint game ids (batch b: ids (3 b + j) x games for setting j), the order rotating.  There is no
threshold on noised against plain games/s: noise spreads the games and lowers the position table's hit rate, which is
the point.  Prints one JSON line per setting and one with the ratios.
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
    ap.add_argument("--batches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    m, eng = make_engine(a.games, a.sims)
    noise = (a.alpha, a.eps, a.draws)
    settings = (("plain", None, "1"), ("plain_turn_loop", None, "0"), ("noised", noise, "1"))
    acc = {name: dict(walls=[], value=0, policy=0, hits=0) for name, _, _ in settings}
    for batch in range(a.warmup + a.batches):
        order = list(enumerate(settings))
        order = order[batch % 3:] + order[:batch % 3]
        for j, (name, rn, one_launch) in order:
            m.game_id_base = (3 * batch + j) * a.games   # (other games every batch and in every setting)
            m.sim_counter = 0
            os.environ["IAGO_PERSISTENT_GAMES"] = one_launch
            before = m._ps["totals"].clone()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.play(a.sims, record=True, root_noise=rn)
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
    os.environ.pop("IAGO_PERSISTENT_GAMES", None)
    out = {}
    for name, rn, _ in settings:
        s, n = acc[name], a.batches * a.games
        out[name] = a.games / statistics.median(s["walls"])
        print(json.dumps(dict(what=name, root_noise=rn, games=a.games, sims=a.sims, batches=a.batches,
                              split_cus=m.split_cus, games_per_s=out[name], games_per_s_all=n / sum(s["walls"]),
                              wall_min=min(s["walls"]), wall_max=max(s["walls"]), value_evals_per_game=s["value"] / n,
                              policy_evals_per_game=s["policy"] / n, table_hits_per_game=s["hits"] / n,
                              replayed=eng.n_replayed)), flush=True)
    print(json.dumps(dict(what="ratios", noised_over_plain_turn_loop=out["noised"] / out["plain_turn_loop"],
                          noised_over_plain=out["noised"] / out["plain"],
                          turn_loop_over_one_launch=out["plain_turn_loop"] / out["plain"])), flush=True)
    m.close()


if __name__ == "__main__":
    main()
