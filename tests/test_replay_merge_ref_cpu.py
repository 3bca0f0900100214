"""The merged replay window without a GPU: the numpy restatement of iago_canonical_rows, iago_replay_merge and
iago_replay_sample_merged (tests/replay_merge_ref.py) against itself -- properties that hold whatever the rows are --
the entry points' place in the header and bindings, and the refusals that come before any device is touched."""
import os
import re

import numpy as np
import pytest
import torch

from iago_amd import _lib
from tests import replay_merge_ref as ref
from tests import replay_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("iago_canonical_rows", "iago_replay_merge", "iago_replay_sample_merged")


@pytest.fixture(scope="module")
def rows():
    return ref.random_game_rows(16, seed=1)


def test_all_eight_variants_share_the_canonical_form(rows):
    c_own, c_opp, sym = ref.canonical(rows["own"], rows["opp"])
    assert sym.dtype == np.uint8 and sym.max() < 8
    for k in range(8):
        o, p, s = ref.canonical(ref.turn_boards(rows["own"], k), ref.turn_boards(rows["opp"], k))
        assert np.array_equal(o, c_own) and np.array_equal(p, c_opp), k
    for i in range(0, rows["own"].size, 7):   # the pair IS variant sym of its row, and no variant is smaller
        pairs = [(int(ref.turn_boards(rows["own"][i:i + 1], k)[0]), int(ref.turn_boards(rows["opp"][i:i + 1], k)[0]))
                 for k in range(8)]
        assert (int(c_own[i]), int(c_opp[i])) == min(pairs) and int(sym[i]) == pairs.index(min(pairs))


def test_the_start_position_ties_four_ways_and_takes_the_lowest():
    own, opp = np.array([0x0000000810000000], np.uint64), np.array([0x0000001008000000], np.uint64)
    pairs = [(int(ref.turn_boards(own, k)[0]), int(ref.turn_boards(opp, k)[0])) for k in range(8)]
    assert sum(p == min(pairs) for p in pairs) == 4
    assert int(ref.canonical(own, opp)[2][0]) == pairs.index(min(pairs))


def test_merged_sums_are_the_rows_sums(rows):
    n = rows["own"].size
    m = ref.merge(rows["own"], rows["opp"], rows["pi"], rows["z"], n)
    assert m["flags"] == 0 and 1 <= m["n_unique"] < n                 # (16 games share their first positions)
    assert int(m["mult"].sum()) == n
    assert np.array_equal(m["first"], np.cumsum(m["mult"]) - m["mult"]) and m["first"].dtype == np.int64
    # the turn into the canonical frame moves counts between cells, not between rows: totals per group and overall
    assert int(m["pi"].astype(np.int64).sum()) == int(rows["pi"].astype(np.int64).sum())
    assert int(m["z_sum"].sum()) == int(rows["z"].astype(np.int64).sum())
    keys = list(zip(m["own"].tolist(), m["opp"].tolist()))
    assert keys == sorted(set(keys))                                  # ascending, unsigned, no group twice
    assert int(m["mult"].max()) == 16                                 # (the start position, once per game)
    # a count below the rows merges the filled slots only
    part = ref.merge(rows["own"], rows["opp"], rows["pi"], rows["z"], 40)
    assert int(part["mult"].sum()) == 40


def test_a_window_without_duplicates_merges_to_its_rows_canonicalised_and_sorted(rows):
    c_own, c_opp, sym = ref.canonical(rows["own"], rows["opp"])
    _, keep = np.unique(np.stack([c_own, c_opp], axis=1), axis=0, return_index=True)
    keep = np.sort(keep)
    own, opp, pi, z = rows["own"][keep], rows["opp"][keep], rows["pi"][keep], rows["z"][keep]
    m = ref.merge(own, opp, pi, z, keep.size)
    assert m["n_unique"] == keep.size and bool((m["mult"] == 1).all())
    order = np.lexsort((c_opp[keep], c_own[keep]))
    assert np.array_equal(m["own"], c_own[keep][order]) and np.array_equal(m["opp"], c_opp[keep][order])
    assert np.array_equal(m["z_sum"], z[order].astype(np.int32))
    for g in range(0, keep.size, 5):
        src = order[g]
        want = replay_ref.apply(own[src], opp[src], pi[src], -1, int(sym[keep][src]))
        assert (int(m["own"][g]), int(m["opp"][g])) == want[:2] and np.array_equal(m["pi"][g], want[2])


def test_sums_beyond_int32_are_clamped_and_flagged():
    own, opp = np.full(3, 0x0000000810000000, np.uint64), np.full(3, 0x0000001008000000, np.uint64)
    pi = np.zeros((3, 64), np.int32)
    pi[:, 19] = 2 ** 30
    m = ref.merge(own, opp, pi, np.ones(3, np.int8), 3)
    assert m["flags"] == ref.OVERFLOW and m["n_unique"] == 1 and int(m["pi"].max()) == 2 ** 31 - 1
    assert ref.merge(own, opp, pi, np.ones(3, np.int8), 1)["flags"] == 0


def test_merged_draws_stay_in_range_and_rows_mode_keeps_the_windows_weights(rows):
    n = rows["own"].size
    m = ref.merge(rows["own"], rows["opp"], rows["pi"], rows["z"], n)
    u = ref.sample(m, n, seed=3, step=0, n=400, mode="unique")
    r = ref.sample(m, n, seed=3, step=0, n=400, mode="rows")
    for s in (u, r):
        assert s["group"].min() >= 0 and s["group"].max() < m["n_unique"] and s["sym"].max() < 8
        assert s["result"].dtype == np.float32 and np.abs(s["result"]).max() <= 1
        assert np.array_equal(s["pi"].sum(axis=1), m["pi"][s["group"]].sum(axis=1))
    # the same Philox words: the variants agree, the groups do not; the largest group is drawn by its weight in rows
    assert np.array_equal(u["sym"], r["sym"]) and not np.array_equal(u["group"], r["group"])
    top = int(np.argmax(m["mult"]))
    assert int((r["group"] == top).sum()) > int((u["group"] == top).sum())
    for j in range(400):                                              # first[g] <= r < first[g] + mult[g]
        row = replay_ref.draw(3, 0, j, n)[0]
        g = int(r["group"][j])
        assert m["first"][g] <= row < m["first"][g] + m["mult"][g]


def test_the_entry_points_are_in_the_training_header_and_the_bindings():
    text = open(os.path.join(ROOT, "include", "iago_hip_training.h")).read()
    declared = set(re.findall(r"IAGO_API[^;(]*?\b(iago_\w+)\s*\(", text))
    core = open(os.path.join(ROOT, "include", "iago_hip.h")).read()
    for name in NEW:
        assert name in declared and name in _lib.TRAINING_SYMBOLS and name not in core, name


def _cpu_window():
    from iago_amd.replay import ReplayWindow
    w = ReplayWindow(capacity=8, device="cpu")
    w.add(dict(own=torch.arange(1, 5), opp=torch.arange(1, 5) << 20, pi=torch.ones((4, 64), dtype=torch.int32),
               move=torch.zeros(4, dtype=torch.int8), z=torch.ones(4, dtype=torch.int8)))
    return w


def test_an_unknown_merged_mode_is_refused_before_any_device():
    w = _cpu_window()
    with pytest.raises(ValueError, match="merged"):
        w.sample(4, merged="x")
    with pytest.raises(ValueError, match="merged"):
        w.sample(4, step=2, merged=True)
    assert w.step == 0                                                # (a refused draw does not advance the counter)


def test_the_move_target_is_refused_with_merged_rows_before_any_device():
    from iago_amd import network
    from iago_amd.train_rl import ReinforceTrainer
    tr = ReinforceTrainer(network.SLPolicy(), pool_dir=None, N=2, seed=1, device="cpu")
    w = _cpu_window()
    for mode in ("unique", "rows"):
        with pytest.raises(ValueError, match="move"):
            tr.step_from_window(w, 4, target="move", merged=mode)
    with pytest.raises(ValueError, match="merged"):
        tr.step_from_window(w, 4, target="visits", merged="x")
    assert w.step == 0 and tr.log == []
