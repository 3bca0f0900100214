"""Times whole self-play games through the turn loop with and without the root values recorded
(SelfPlayEngine.play(root_values=True): one more small launch per turn, iago_mcts_root_value, and two more record columns),
the shipped nets under the negamax backup, one engine, one process.

    python tools/time_root_values.py [--games 256] [--sims 100] [--out profiles/root_values_bench.json]

Both arms play the SAME games through the SAME path: root_noise=(77, 0) -- noise mixed with weight 0, which plays the
plain games -- sends the arm without the record through the turn loop too, and the arm with the record takes it as well,
so the only difference is the record.  The same game ids and the same sim_counter in every run; one warm-up run of those
games first, so that both arms meet the position table as a run of the same games left it.  ONE run per arm, both on
the same box, the arm without the record first.  There is no threshold: the ratio is stated as measured.  The moves and
results of the two arms are compared, and the JSON line says whether they are the same games.  Prints the JSON line and
writes it to --out.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.time_backup import make_engine  # noqa: E402

NOISE = (77, 0)


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(root, "profiles", "root_values_bench.json"))
    a = ap.parse_args()
    m, eng = make_engine(a.games, a.sims, "negamax")

    def run(root_values):
        m.sim_counter = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = eng.play(a.sims, record=True, root_noise=NOISE, root_values=root_values)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    run(False)                                   # warm-up: the kernels, the position table
    wall_off, off = run(False)
    wall_on, on = run(True)
    same = all(torch.equal(getattr(on, k), getattr(off, k)) for k in ("move", "valid", "z", "pi"))
    searched = int(((on.valid == 1) | (on.valid == 4)).sum().item())
    out = dict(what="self-play through the turn loop, root values recorded against not recorded, one run per arm",
               games=a.games, sims=a.sims, root_noise=NOISE, backup="negamax", turns=on.n_turns,
               launches=[off.launches, on.launches], searched_rows=searched, same_games=same,
               wall_s_without=wall_off, wall_s_with=wall_on, games_per_s_without=a.games / wall_off,
               games_per_s_with=a.games / wall_on, with_over_without_wall=wall_on / wall_off,
               extra_ms_per_turn=1e3 * (wall_on - wall_off) / on.n_turns)
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    m.close()


if __name__ == "__main__":
    main()
