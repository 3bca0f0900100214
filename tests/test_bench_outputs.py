"""bench.py --dump-outputs on the host: bitboards survive as float64 halves, every array is float32 / float64, and a
result beyond the size limit is written as a fixed sample of its games (CPU)."""
import os
import types

import numpy as np
import torch

import bench


def fake_result(T, B, seed):
    g = torch.Generator().manual_seed(seed)
    r = types.SimpleNamespace()
    r.own = torch.randint(-2 ** 62, 2 ** 62, (T, B), dtype=torch.int64, generator=g)
    r.opp = torch.randint(-2 ** 62, 2 ** 62, (T, B), dtype=torch.int64, generator=g)
    r.own[0, 0], r.opp[0, 0] = -1, -2 ** 63       # every bit / the sign bit alone
    r.pi = torch.randint(0, 500, (T, B, 64), dtype=torch.int32, generator=g)
    r.valid = torch.randint(0, 2, (T, B), dtype=torch.uint8, generator=g)
    r.move = torch.randint(-1, 64, (T, B), dtype=torch.int8, generator=g)
    r.z = torch.randint(-1, 2, (B,), dtype=torch.int8, generator=g)
    r.final_p1, r.final_p2 = r.own[-1].clone(), r.opp[-1].clone()
    r.game_turns = torch.randint(1, T + 1, (B,), dtype=torch.int32, generator=g)
    return r


def load_all(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_outputs_exact_and_within_the_limit(tmp_path):
    r = fake_result(12, 40, seed=1)
    out = bench.selfplay_outputs(r)
    bench.dump_outputs(str(tmp_path / "all"), out)
    got = load_all(str(tmp_path / "all"))
    assert set(got) == {"games", "own", "opp", "pi", "valid", "move", "z", "final_p1", "final_p2", "game_turns"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["games"], np.arange(40))
    for name in ("own", "opp", "final_p1", "final_p2"):
        h = got[name].astype(np.uint64)
        back = (h[..., 0] | (h[..., 1] << np.uint64(32))).view(np.int64)
        assert np.array_equal(back, getattr(r, name).numpy()), name
    assert np.array_equal(got["pi"], r.pi.numpy()) and np.array_equal(got["move"], r.move.numpy())
    # beyond the limit: a seeded sample of the games, the same one every time, every array cut along its game axis
    limit = 40 * 1024
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), out, limit=limit)
    s1, s2 = load_all(str(tmp_path / "s1")), load_all(str(tmp_path / "s2"))
    keep = s1["games"].astype(np.int64)
    assert 0 < len(keep) < 40 and np.array_equal(keep, np.unique(keep))
    assert sum(os.path.getsize(str(tmp_path / "s1" / f)) for f in os.listdir(str(tmp_path / "s1"))) <= limit
    for name in s1:
        assert np.array_equal(s1[name], s2[name]), name
    assert np.array_equal(s1["pi"], r.pi.numpy()[:, keep]) and np.array_equal(s1["z"], r.z.numpy()[keep])
    assert np.array_equal(s1["game_turns"], r.game_turns.numpy()[keep])
