"""Times whole self-play games under both selection rules (engine.BatchedMCTS(selection="reference" | "alphazero")), the
shipped nets, the two settings interleaved batch by batch in one process.

    python tools/time_selection.py [--games 1024] [--sims 100] [--batches 20] [--warmup 2] [--backup reference]

Two engines on the same nets, each with its own tree pool and position table (a stored value is a function of the
position alone, but which positions a search meets is the rule's).  Disjoint game ids (batch b: ids (2 b + j) x games
for setting j), the order alternating.  The trees differ -- the AlphaZero rule's are narrower and deeper, so its descents
are longer --, so the times do: this is a record, not a bar.  Prints one JSON
line per rule -- games/s over the median batch, leaf evaluations/s (playouts backed up: games x searched turns x sims
over the wall time), net evaluations and table hits per game -- and one with the ratio.
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


def make_engine(n_games, n_sims, selection, backup, seed=7):
    policy = network.SLPolicy().load_npz(os.path.join(GOLDEN, "sl_model.npz")).cuda().eval()
    value = network.Value().load_npz(os.path.join(GOLDEN, "value_model.npz")).cuda().eval()
    value.split_f16 = True
    with open(os.path.join(GOLDEN, "simulate.json")) as f:
        g = json.load(f)
    m = engine.BatchedMCTS(n_games, policy, value, ops.RolloutWeights(g["shipped_w"], g["shipped_b"]), lmbda=0.5,
                           c_puct=1.0, n_thr=15, seed=seed, persistent=True, backup=backup, selection=selection,
                           capacity=engine.suggest_capacity(n_sims, 15, moves=64))
    m.warmup()
    return m, engine.SelfPlayEngine(m, max_turns=128)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--backup", default="reference")
    a = ap.parse_args()
    settings = [(rule,) + make_engine(a.games, a.sims, rule, a.backup) for rule in engine.SELECTION_RULES]
    acc = {rule: dict(walls=[], value=0, policy=0, hits=0, evals=0) for rule, _, _ in settings}
    for batch in range(a.warmup + a.batches):
        order = list(enumerate(settings))
        order = order[batch % 2:] + order[:batch % 2]
        for j, (rule, m, eng) in order:
            m.game_id_base = (2 * batch + j) * a.games   # (other games every batch and in every setting)
            m.sim_counter = 0
            before, evals = m._ps["totals"].clone(), m.n_leaf_evals
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.play(a.sims, record=True)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            if batch < a.warmup:
                continue
            d = (m._ps["totals"] - before).tolist()
            s = acc[rule]
            s["walls"].append(wall)
            s["value"] += d[0]
            s["policy"] += d[1]
            s["hits"] += d[8]
            s["evals"] += m.n_leaf_evals - evals
    out = {}
    for rule, m, eng in settings:
        s, n = acc[rule], a.batches * a.games
        out[rule] = a.games / statistics.median(s["walls"])
        print(json.dumps(dict(what=rule, backup=m.backup, games=a.games, sims=a.sims, batches=a.batches, split_cus=m.split_cus,
                              games_per_s=out[rule], games_per_s_all=n / sum(s["walls"]),
                              leaf_evals_per_s=s["evals"] / sum(s["walls"]), wall_min=min(s["walls"]),
                              wall_max=max(s["walls"]), value_evals_per_game=s["value"] / n,
                              policy_evals_per_game=s["policy"] / n, table_hits_per_game=s["hits"] / n,
                              replayed=eng.n_replayed)), flush=True)
        m.close()
    print(json.dumps(dict(what="ratios", alphazero_over_reference=out["alphazero"] / out["reference"])), flush=True)


if __name__ == "__main__":
    main()
