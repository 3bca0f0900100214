"""Times self-play under the Gumbel root search against the plain search (SelfPlayEngine.play(n, gumbel=(m, c_scale_256))
against play(n)), the shipped nets under the negamax backup and the AlphaZero selection, both through the turn loop
(IAGO_PERSISTENT_GAMES=0 is set here: the rule has no whole-game launch, so the ratio is the cost of the rule -- the draw
and the finish launches per turn, the fresh roots, the root's reductions -- not of the turn loop), the two settings
interleaved batch by batch in one process, at every playout count of --sims.

    python tools/time_gumbel.py [--games 1024] [--sims 16,100] [--m 16] [--c-scale 256] [--n-thr 1] [--batches 6]
                                [--warmup 2] [--out profiles/gumbel_bench.json]

Every setting meets the position table as the earlier batches of both settings left it, never its own games: disjoint
game ids (batch b: ids (2 b + j) x games for setting j), the order alternating.  There is no threshold on the ratio: it
is reported.  Prints one JSON line per setting and playout count and writes them all to --out."""
import argparse
import json
import os
import statistics
import sys
import time

os.environ["IAGO_PERSISTENT_GAMES"] = "0"

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def make_engine(n_games, n_sims, n_thr, seed=7):
    from iago_amd import engine, network, ops
    policy = network.SLPolicy().load_npz(os.path.join(GOLDEN, "sl_model.npz")).cuda().eval()
    value = network.Value().load_npz(os.path.join(GOLDEN, "value_model.npz")).cuda().eval()
    value.split_f16 = True
    with open(os.path.join(GOLDEN, "simulate.json")) as f:
        g = json.load(f)
    m = engine.BatchedMCTS(n_games, policy, value, ops.RolloutWeights(g["shipped_w"], g["shipped_b"]), lmbda=0.5, c_puct=1.0,
                           n_thr=n_thr, seed=seed, persistent=True, backup="negamax", selection="alphazero",
                           capacity=engine.suggest_capacity(n_sims, n_thr, moves=64))
    m.warmup()
    return m, engine.SelfPlayEngine(m, max_turns=128)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--sims", default="16,100")
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--c-scale", type=int, default=256)
    ap.add_argument("--n-thr", type=int, default=1)
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gumbel_bench.json"))
    a = ap.parse_args()
    lines = []
    for sims in (int(s) for s in a.sims.split(",")):
        m, eng = make_engine(a.games, sims, a.n_thr)
        settings = (("plain", None), ("gumbel", (a.m, a.c_scale)))
        walls = {name: [] for name, _ in settings}
        turns = {name: 0 for name, _ in settings}
        for batch in range(a.warmup + a.batches):
            order = list(enumerate(settings))
            order = order[batch % 2:] + order[:batch % 2]
            for j, (name, gumbel) in order:
                m.game_id_base = (2 * batch + j) * a.games   # (other games every batch and in every setting)
                m.sim_counter = 0
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = eng.play(sims, record=True, gumbel=gumbel)
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0
                assert res.launches == res.n_turns   # (the turn loop)
                if batch >= a.warmup:
                    walls[name].append(wall)
                    turns[name] += res.n_turns
        out = {}
        for name, gumbel in settings:
            w = walls[name]
            out[name] = a.games / statistics.median(w)
            lines.append(dict(what=name, gumbel=list(gumbel) if gumbel else None, games=a.games, sims=sims, n_thr=a.n_thr,
                              batches=a.batches, split_cus=m.split_cus, games_per_s=round(out[name], 1),
                              games_per_s_all=round(a.batches * a.games / sum(w), 1), wall_min=round(min(w), 4),
                              wall_max=round(max(w), 4), turns_per_batch=turns[name] / a.batches,
                              device=torch.cuda.get_device_name(0)))
            print(json.dumps(lines[-1]), flush=True)
        lines.append(dict(what="ratio", sims=sims, gumbel_over_plain=round(out["gumbel"] / out["plain"], 4)))
        print(json.dumps(lines[-1]), flush=True)
        m.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
