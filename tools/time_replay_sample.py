#!/usr/bin/env python3
"""ReplayWindow.sample(rows) out of a full window against the same minibatch restated in tensor operations: the drawn
slots and variants taken as given, index_select of the five columns, the visit rows gathered through a precomputed
[8][64] permutation table, the boards and moves through ops.augment8 of the selected rows and a pick of each row's
variant.  Device time per call (events around `reps` calls), and the two results compared.  One JSON line.
--merged: every row of the window is one of window / 4 positions in a random symmetry (a window with duplicates), and
the line also carries the merged draws of the same `rows` rows (iago_replay_sample_merged, both modes, through ops and
through ReplayWindow.sample(merged=) on its kept snapshot), ReplayWindow.merge()'s wall time and n_unique.
    python3 tools/time_replay_sample.py [window=262144] [rows=4096] [reps=200] [--merged]"""
import json, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from iago_amd import ops  # noqa: E402
from iago_amd.replay import ReplayWindow  # noqa: E402

with_merged = "--merged" in sys.argv
argv = [x for x in sys.argv if x != "--merged"]
arg = lambda i, d: int(argv[i]) if len(argv) > i else d  # noqa: E731
capacity, rows, reps = arg(1, 262144), arg(2, 4096), arg(3, 200)
g = torch.Generator().manual_seed(0)
w = ReplayWindow(capacity, seed=3)
own = torch.randint(-2 ** 63, 2 ** 63 - 1, (capacity,), generator=g, dtype=torch.int64)
opp = torch.randint(-2 ** 63, 2 ** 63 - 1, (capacity,), generator=g, dtype=torch.int64) & ~own
if with_merged:
    pick = torch.randint(0, max(capacity // 4, 1), (capacity,), generator=g)
    turned = ops.augment8(own[pick].cuda(), opp[pick].cuda(), torch.zeros(capacity, dtype=torch.int8, device="cuda"))
    k = torch.randint(0, 8, (1, capacity), generator=g).cuda()
    own, opp = turned[0].gather(0, k)[0], turned[1].gather(0, k)[0]
w.add(dict(own=own, opp=opp, pi=torch.randint(0, 100, (capacity, 64), generator=g, dtype=torch.int32),
           move=torch.randint(-1, 64, (capacity,), generator=g, dtype=torch.int8),
           z=torch.randint(-1, 2, (capacity,), generator=g, dtype=torch.int8)))

# inverse[k][d] = the source cell of destination d in variant k, from augment8 of the 64 one-cell rows
cells = torch.arange(64, dtype=torch.int8, device="cuda")
zero = torch.zeros(64, dtype=torch.int64, device="cuda")
m = ops.augment8(zero, zero, cells)[2].to(torch.int64)          # (8, 64): m[k][a]
inverse = torch.empty_like(m)
inverse.scatter_(1, m, torch.arange(64, device="cuda").expand(8, 64).contiguous())


def restated(slot, sym):
    s, k = slot.to(torch.int64), sym.to(torch.int64)
    c = w.cols
    o8, p8, a8 = ops.augment8(c["own"].index_select(0, s), c["opp"].index_select(0, s), c["move"].index_select(0, s))
    pick = k.reshape(1, -1)
    z = c["z"].index_select(0, s)
    return dict(own=o8.gather(0, pick)[0], opp=p8.gather(0, pick)[0], move=a8.gather(0, pick)[0],
                pi=c["pi"].index_select(0, s).gather(1, inverse.index_select(0, k)), z=z, result=z.to(torch.float32))


def timed(fn):
    for _ in range(10):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


first = w.sample(rows, step=0)
again = restated(first["slot"], first["sym"])
same = all(torch.equal(first[k], again[k]) for k in again)
c = w.cols
t_sample = timed(lambda: w.sample(rows, step=0))                 # (with the window's read-back of its flag word)
t_kernel = timed(lambda: ops.replay_sample(c["own"], c["opp"], c["pi"], c["move"], c["z"], w.count, n=rows, seed=3))
t_torch = timed(lambda: restated(first["slot"], first["sym"]))
extra = {}
if with_merged:
    import time
    walls = []
    for _ in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = w.merge()
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    extra = {"n_unique": m.n_unique, "largest_group": int(m.mult.max().item()), "merge_wall_ms": min(walls[1:])}
    for mode in ("unique", "rows"):
        extra["ops_replay_sample_merged_%s_us" % mode] = timed(lambda: ops.replay_sample_merged(
            m.own, m.opp, m.pi, m.z_sum, m.mult, m.first, m.count, rows, seed=3, mode=mode))
        extra["window_sample_merged_%s_us" % mode] = timed(lambda: w.sample(rows, step=0, merged=mode))
print(json.dumps({"window_rows": capacity, "rows": rows, "reps": reps, "restatement_equal": bool(same),
                  "window_sample_us": t_sample, "ops_replay_sample_us": t_kernel, "torch_restatement_us": t_torch,
                  "bytes_moved": rows * 2 * 290, "kernel_GBps": rows * 2 * 290 / (t_kernel * 1e-6) / 1e9, **extra}))
