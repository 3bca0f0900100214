"""Times the wave search (engine.BatchedMCTS(wave=W), iago_mcts_search_wave) on ONE game from the start position.

    python tools/time_wave.py [--sims 200,3200] [--waves 1,8,16,32] [--vloss 0,1] [--reps 3] [--out FILE]

Per (playouts per search, W, vloss): a fresh tree per search (iago_mcts_reset), `reps` timed searches after one
warm-up; playouts/s, the time to 6,600 playouts (about the reference's 10-second move), and the game workgroup's time
split into descents / rollouts / backups / waiting for a net (the library's wave_timing, 100 MHz ticks).  "persistent"
is today's search (iago_mcts_search_persistent, one playout of the tree in flight); W = 1 runs the wave entry point.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from iago_amd import engine, network, ops  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


def nets():
    policy = network.SLPolicy().load_npz(os.path.join(GOLDEN, "sl_model.npz")).cuda().eval()
    value = network.Value().load_npz(os.path.join(GOLDEN, "value_model.npz")).cuda().eval()
    g = json.load(open(os.path.join(GOLDEN, "simulate.json")))
    return policy, value, ops.RolloutWeights(g["shipped_w"], g["shipped_b"])


def run(policy, value, rw, n_sims, wave, vloss, reps, entry):
    m = engine.BatchedMCTS(1, policy, value, rw, lmbda=0.5, c_puct=1.0, n_thr=15, capacity=1 << 18, seed=1,
                           wave=wave, virtual_loss=vloss)
    m.wave_entry = entry
    own, opp = ops.bits_to_tensor([0x0000000810000000]), ops.bits_to_tensor([0x0000001008000000])
    one = torch.ones(1, dtype=torch.uint8, device="cuda")
    m.tree.reset()
    m.search(own, opp, one, n_sims)   # warm-up (and the position table's first fill: every search below meets it)
    m.wave_timing.zero_()
    times = []
    for _ in range(reps):
        m.tree.reset()
        torch.cuda.synchronize()
        t = time.perf_counter()
        m.search(own, opp, one, n_sims)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t)
    best = min(times)
    tick = [int(x) for x in m.wave_timing.tolist()]
    total = max(sum(tick), 1)
    return dict(n_sims=n_sims, wave=wave if entry else "persistent", vloss=vloss, s_per_search=best,
                playouts_per_s=n_sims / best, s_to_6600=6600 * best / n_sims, move=int(m.best_move(one)[0].item()),
                gw_us_per_search=dict(descent=tick[0] / 100.0 / reps, rollout=tick[1] / 100.0 / reps,
                                      backup=tick[2] / 100.0 / reps, wait=tick[3] / 100.0 / reps),
                gw_share=dict(descent=tick[0] / total, rollout=tick[1] / total, backup=tick[2] / total,
                              wait=tick[3] / total))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sims", default="200,3200")
    ap.add_argument("--waves", default="1,8,16,32")
    ap.add_argument("--vloss", default="0,1")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    policy, value, rw = nets()
    rows = []
    for n_sims in (int(x) for x in a.sims.split(",")):
        rows.append(run(policy, value, rw, n_sims, 1, 1.0, a.reps, False))
        print(json.dumps(rows[-1]), flush=True)
        for wave in (int(x) for x in a.waves.split(",")):
            for vloss in ((1.0,) if wave == 1 else tuple(float(x) for x in a.vloss.split(","))):
                rows.append(run(policy, value, rw, n_sims, wave, vloss, a.reps, True))
                print(json.dumps(rows[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(rows, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
