"""One epoch of Value-net training (train_value.py: minibatches of 4,096, Chainer's Adam + WeightDecay) over 65,536
samples, SupervisedTrainer(native=True) -- the split-f16 gradient kernels -- against native=False -- autograd over the
tensor library's float32 convolutions.

    python tools/time_value_train.py [--rounds R] [--samples N]

Both arms are warmed up first (an epoch each: the autograd arm's first epoch includes the convolution library's
solver search, reported on its own), then the arms alternate R times within this one process; every epoch is timed
with a host clock around a device synchronise.  Also: the gradients of one 4,096-row minibatch (Value.value_grads)
next to the REINFORCE update's gradients of 1,900 rows (SLPolicy.reinforce_grads).  Prints one JSON line at the end.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from iago_amd import network, rl_self_play  # noqa: E402
from iago_amd.train_supervised import MINIBATCH, SupervisedTrainer  # noqa: E402


def rows(n, seed=1):
    """n positions of policy-vs-policy games (own = the side to move), their moves and a result in {-1, 1}."""
    torch.manual_seed(seed)
    m = network.SLPolicy().cuda().eval()
    r = rl_self_play.play_batch(m, m, 1024, seed=seed)
    valid = r["action"] >= 0
    z = r["z"].reshape(1, -1).expand_as(r["action"])
    own, opp, act, zz = r["own"][valid], r["opp"][valid], r["action"][valid], z[valid].to(torch.float32)
    reps = (n + own.numel() - 1) // own.numel()
    return [t.repeat(reps)[:n].contiguous() for t in (own, opp, act, zz)]


def clock(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--samples", type=int, default=65536)
    a = ap.parse_args()
    own, opp, act, y = rows(a.samples)
    torch.manual_seed(0)
    nets = {"native": network.Value().cuda(), "autograd": network.Value().cuda()}
    nets["autograd"].load_state_dict(nets["native"].state_dict())
    trainers = {k: SupervisedTrainer(m, "value", seed=1, native=(k == "native")) for k, m in nets.items()}
    warm = {k: clock(lambda t=t: t.epoch(own, opp, y)) for k, t in trainers.items()}
    times = {k: [] for k in trainers}
    for _ in range(a.rounds):
        for k, t in trainers.items():
            times[k].append(clock(lambda t=t: t.epoch(own, opp, y)))
    # the gradients alone: one minibatch of the Value net, and the REINFORCE update's 1,900 rows of SLPolicy
    v = nets["native"]
    mb = slice(0, MINIBATCH)
    keep = torch.rand((MINIBATCH, 128), device="cuda") >= 0.4
    pol = network.SLPolicy().cuda()
    g_value, g_policy = [], []
    for _ in range(max(a.rounds, 5) + 1):
        g_value.append(clock(lambda: v.value_grads(own[mb], opp[mb], y[mb], keep=keep)))
        g_policy.append(clock(lambda: pol.reinforce_grads(own[:1900], opp[:1900], act[:1900], y[:1900])))
    g_value, g_policy = g_value[1:], g_policy[1:]
    steps = (a.samples + MINIBATCH - 1) // MINIBATCH
    out = dict(samples=a.samples, minibatches=steps, rounds=a.rounds,
               warmup_s={k: round(w, 4) for k, w in warm.items()},
               epoch_s={k: {q: (round(x, 5) if isinstance(x, float) else x) for q, x in spread(ts).items()}
                        for k, ts in times.items()},
               speedup=round(statistics.median(times["autograd"]) / statistics.median(times["native"]), 3),
               value_grads_ms_4096={q: (round(x * 1e3, 3) if isinstance(x, float) else x)
                                    for q, x in spread(g_value).items()},
               policy_grads_ms_1900={q: (round(x * 1e3, 3) if isinstance(x, float) else x)
                                     for q, x in spread(g_policy).items()},
               device=torch.cuda.get_device_name())
    for k in times:
        s = spread(times[k])
        print("%-8s epoch of %d samples (%d minibatches): median %.1f ms (min %.1f, max %.1f over %d); first epoch "
              "%.2f s" % (k, a.samples, steps, s["median"] * 1e3, s["min"] * 1e3, s["max"] * 1e3, s["n"], warm[k]))
    print("gradients: Value %.2f ms per %d rows, SLPolicy REINFORCE %.2f ms per 1,900 rows (medians)"
          % (statistics.median(g_value) * 1e3, MINIBATCH, statistics.median(g_policy) * 1e3))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
