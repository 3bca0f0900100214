"""Times whole self-play games with and without playout-cap randomisation (SelfPlayEngine.play(playout_cap=(n_fast,
full_per_256))), the shipped nets, the two settings interleaved batch by batch in one process.

    python tools/time_playout_cap.py [--games 1024] [--sims 100] [--fast 25] [--full 64] [--batches 20] [--warmup 5]
                                     [--cold]

Both settings meet the same position-table state.  The table outlives play(), and a fast turn is the first n_fast
playouts of the full turn's search: a capped batch played after the plain batch of the SAME games would find its values
stored.  So the two settings play disjoint game ids (batch b: ids (2 b + j) x games for setting j) and take turns at
going first: each finds the table as the earlier batches of both left it, never its own games.  --cold empties the
table before every batch instead (outside the timed span): what a first batch pays.

Prints one JSON line per setting: games/s (median batch and all batches), value and policy evaluations per game, the
net workgroups' busy share (walking / (walking + waiting) of totals[5] / totals[4]), searched full / fast rows per
game; then one line with the capped speed-up against the playout ratio p + (1 - p) n_fast / n_sims.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from iago_amd import engine, network, ops  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


def make_engine(n_games, n_sims, seed=7):
    policy = network.SLPolicy().load_npz(os.path.join(GOLDEN, "sl_model.npz")).cuda().eval()
    value = network.Value().load_npz(os.path.join(GOLDEN, "value_model.npz")).cuda().eval()
    value.split_f16 = True
    with open(os.path.join(GOLDEN, "simulate.json")) as f:
        g = json.load(f)
    m = engine.BatchedMCTS(n_games, policy, value, ops.RolloutWeights(g["shipped_w"], g["shipped_b"]), lmbda=0.5,
                           c_puct=1.0, n_thr=15, seed=seed, persistent=True,
                           capacity=engine.suggest_capacity(n_sims, 15, moves=64))
    m.warmup()
    return m, engine.SelfPlayEngine(m, max_turns=128)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--fast", type=int, default=25)
    ap.add_argument("--full", type=int, default=64)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cold", action="store_true")
    a = ap.parse_args()
    m, eng = make_engine(a.games, a.sims)
    settings = (("plain", None), ("capped", (a.fast, a.full)))
    acc = {name: dict(walls=[], value=0, policy=0, wait=0, walk=0, full=0, fast=0) for name, _ in settings}
    for batch in range(a.warmup + a.batches):
        for j, (name, cap) in list(enumerate(settings))[::1 if batch % 2 == 0 else -1]:
            m.game_id_base = (2 * batch + j) * a.games   # (other games every batch and in either setting)
            m.sim_counter = 0
            if a.cold and m._vtable is not None:
                m._vtable.zero_()
            before = m._ps["totals"].clone()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = eng.play(a.sims, record=True, playout_cap=cap)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            if batch < a.warmup:
                continue
            d = (m._ps["totals"] - before).tolist()
            s = acc[name]
            s["walls"].append(wall)
            s["value"] += d[0]
            s["policy"] += d[1]
            s["wait"] += d[4]
            s["walk"] += d[5]
            s["full"] += int((res.valid == 1).sum())
            s["fast"] += int((res.valid == 4).sum())
    out = {}
    for name, cap in settings:
        s, n = acc[name], a.batches * a.games
        out[name] = a.games / statistics.median(s["walls"])
        print(json.dumps(dict(what=name, playout_cap=cap, games=a.games, sims=a.sims, batches=a.batches,
                              table="cold" if a.cold else "shared", split_cus=m.split_cus,
                              games_per_s=out[name], games_per_s_all=n / sum(s["walls"]),
                              wall_min=min(s["walls"]), wall_max=max(s["walls"]),
                              value_evals_per_game=s["value"] / n, policy_evals_per_game=s["policy"] / n,
                              net_busy_share=s["walk"] / max(1, s["walk"] + s["wait"]),
                              full_rows_per_game=s["full"] / n, fast_rows_per_game=s["fast"] / n,
                              replayed=eng.n_replayed)), flush=True)
    p = a.full / 256
    print(json.dumps(dict(what="speed-up", capped_over_plain=out["capped"] / out["plain"],
                          playout_ratio=p + (1 - p) * a.fast / a.sims)), flush=True)
    m.close()


if __name__ == "__main__":
    main()
