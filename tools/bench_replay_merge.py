#!/usr/bin/env python3
"""How much of a real self-play window is duplicate positions, and what merging it costs.  The window is filled from
whole exploring rounds -- SelfPlayEngine.play(sims, explore_turns=8) with the shipped nets, `games` lockstep games a
round, every round under game ids of its own (the explore draws are keyed by the game id) -- until it holds `rows` rows,
then measured:
  unique_share          n_unique / count of ReplayWindow.merge(), overall and per turn 0 .. 12 (a row's turn is its
                        game's turn counter), with the five largest groups;
  merge_ms              wall time of ReplayWindow.merge() (canonical forms, two sorts, the reduction, one readback),
                        median of `reps` after one warm-up, beside round_s, the median wall time of one round's
                        self-play in the same run: a merge happens once per round;
  merge_device_ms       device time of ops.replay_merge alone (events), and of ops.canonical_rows alone;
  draw_us               device time per call of a 1,024-row draw: iago_replay_sample against iago_replay_sample_merged
                        in both modes, on this window.
One JSON object per window size, appended to --out as a JSON list.
    python3 tools/bench_replay_merge.py [--rows 65536] [--games 1024] [--sims 100] [--reps 5] [--out FILE]"""
import argparse, json, os, statistics, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from iago_amd import engine, network, ops  # noqa: E402
from iago_amd.replay import ReplayWindow  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=65536)
ap.add_argument("--games", type=int, default=1024)
ap.add_argument("--sims", type=int, default=100)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--draw-rows", type=int, default=1024)
ap.add_argument("--out", default=None)
a = ap.parse_args()

policy = network.SLPolicy().load_npz(os.path.join(GOLDEN, "sl_model.npz")).cuda().eval()
value = network.Value().load_npz(os.path.join(GOLDEN, "value_model.npz")).cuda().eval()
with open(os.path.join(GOLDEN, "simulate.json")) as f:
    g = json.load(f)
m = engine.BatchedMCTS(a.games, policy, value, ops.RolloutWeights(g["shipped_w"], g["shipped_b"]), n_thr=15, seed=1,
                       capacity=engine.suggest_capacity(a.sims, 15))
sp = engine.SelfPlayEngine(m)
window = ReplayWindow(a.rows, seed=3)
turns, round_s, rounds = [], [], 0
while window.total < a.rows:
    m.game_id_base = rounds * a.games
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tup = sp.play(a.sims, explore_turns=8).tuples()
    torch.cuda.synchronize()
    round_s.append(time.perf_counter() - t0)
    # the last round is cut to the WHOLE games that still fit (tuples() come turn by turn: a cut by rows would keep the
    # opening turns of every game and nothing else), so the window ends up to a game's rows short of `rows`
    game = tup["game"].to(torch.int64) - m.game_id_base
    fit = int((torch.cumsum(torch.bincount(game, minlength=a.games), 0) <= a.rows - window.total).sum())
    keep = game < fit
    window.add({k: tup[k][keep] for k in ("own", "opp", "pi", "move", "z")})
    turns.append(tup["turn"][keep].to(torch.int64))
    rounds += 1
    print("round %d: %.2f s, %d rows" % (rounds, round_s[-1], window.total), file=sys.stderr, flush=True)
    if fit < a.games:
        break
m.close()
turns = torch.cat(turns)
c = window.cols


def wall_ms(fn, reps):
    out = []
    for rep in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if rep:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def device_us(fn, reps):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


merged = window.merge()
merge_ms = wall_ms(window.merge, a.reps)
merge_dev = device_us(lambda: ops.replay_merge(c["own"], c["opp"], c["pi"], c["z"], window.count), a.reps) / 1e3
filled = c["own"][:window.count], c["opp"][:window.count]
canon_dev = device_us(lambda: ops.canonical_rows(*filled), a.reps) / 1e3
c_own, c_opp, _ = ops.canonical_rows(*filled)
per_turn = []
for t in range(13):
    at = turns == t
    n = int(at.sum())
    u = int(torch.unique(torch.stack([c_own[at], c_opp[at]], dim=1), dim=0).shape[0]) if n else 0
    per_turn.append(dict(turn=t, rows=n, unique=u))
n = a.draw_rows
draw = dict(
    replay_sample=device_us(lambda: ops.replay_sample(c["own"], c["opp"], c["pi"], c["move"], c["z"], window.count, n=n,
                                                      seed=3), 200),
    **{"merged_" + mode: device_us(lambda: ops.replay_sample_merged(merged.own, merged.opp, merged.pi, merged.z_sum,
                                                                    merged.mult, merged.first, merged.count, n, seed=3,
                                                                    mode=mode), 200) for mode in ("unique", "rows")})
z_mean = merged.z_sum.to(torch.float64) / merged.mult.to(torch.float64)
top = torch.sort(merged.mult, descending=True)[0][:5].tolist()
out = dict(config="play(%d, explore_turns=8), %d games a round, shipped nets, game ids of its own per round, 1 x MI355X"
                  % (a.sims, a.games),
           rows=window.count, rounds=rounds, n_unique=merged.n_unique, unique_share=merged.n_unique / window.count,
           duplicate_rows=window.count - merged.n_unique, largest_groups=top, per_turn=per_turn,
           opening_mean_result=float(z_mean[int(torch.argmax(merged.mult))].item()),
           round_s=statistics.median(round_s), round_s_all=round_s,
           merge_ms=statistics.median(merge_ms), merge_ms_all=merge_ms, merge_device_ms=merge_dev,
           canonical_rows_device_ms=canon_dev, merge_share_of_round=statistics.median(merge_ms) / 1e3 / statistics.median(round_s),
           draw_rows=n, draw_us=draw)
print(json.dumps(out))
if a.out:
    prior = json.load(open(a.out)) if os.path.exists(a.out) else []
    with open(a.out, "w") as f:
        json.dump(prior + [out], f, indent=1)
        f.write("\n")
