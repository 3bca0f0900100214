"""The merged replay window on the GPU (iago_canonical_rows, iago_replay_merge, iago_replay_sample_merged; ops.
canonical_rows / replay_merge / replay_sample_merged, ReplayWindow.merge / sample(merged=), ReinforceTrainer.
step_from_window(merged=)) against tests/replay_merge_ref.py, output for output and bit for bit: everything is in
integers but one float32 division.  The rows are those of 64 seeded uniformly random games on the oracle's rules
(about 3,800): they share the start position and its successors, so groups of 64 rows and positions that are their own
mirror image come with them -- both asserted, so that the data cannot quietly stop exercising either."""
import numpy as np
import pytest
import torch

from tests import replay_merge_ref as ref

pytestmark = pytest.mark.gpu

START = (0x0000000810000000, 0x0000001008000000)
MERGED = ("own", "opp", "pi", "z_sum", "mult", "first")
DRAWN = ("group", "sym", "own", "opp", "pi", "result", "z_sum", "mult")


@pytest.fixture(scope="module")
def rows():
    r = ref.random_game_rows(64, seed=0)
    assert 3000 < r["own"].size < 3841
    return r


def _window(r, capacity=None, seed=4):
    from iago_amd.replay import ReplayWindow
    n = r["own"].size
    w = ReplayWindow(capacity or n, seed=seed)
    w.add(_tup(r, 0, n))
    return w


def _tup(r, lo, hi):
    from iago_amd import ops
    return dict(own=ops.bits_to_tensor(r["own"][lo:hi]), opp=ops.bits_to_tensor(r["opp"][lo:hi]),
                pi=torch.from_numpy(np.ascontiguousarray(r["pi"][lo:hi])), z=torch.from_numpy(r["z"][lo:hi].copy()),
                move=torch.full((hi - lo,), -1, dtype=torch.int8))


def _host(w):
    """The window's columns as the restatement takes them."""
    c = {k: v.cpu().numpy() for k, v in w.cols.items()}
    return c["own"].view(np.uint64), c["opp"].view(np.uint64), c["pi"], c["z"], w.count


def _same(got, exp, keys):
    for k in keys:
        have = got[k] if isinstance(got, dict) else getattr(got, k)
        have = have.cpu().numpy()
        if k in ("own", "opp"):
            have = have.view(np.uint64)
        assert have.dtype == exp[k].dtype and have.shape == exp[k].shape and np.array_equal(have, exp[k]), k


@pytest.fixture(scope="module")
def merged_rows(rows):
    """(the window of all fixture rows, its merge on the device, the restatement's) -- computed once."""
    w = _window(rows)
    return w, w.merge(), ref.merge(*_host(w))


def test_the_fixture_has_a_large_group_and_a_self_symmetric_position(merged_rows):
    exp = merged_rows[2]
    assert int(exp["mult"].max()) >= 32
    assert int((exp["mult"] > 1).sum()) > 20 and exp["n_unique"] < merged_rows[0].count
    mirrored = np.zeros(exp["n_unique"], dtype=bool)
    for k in range(1, 8):
        mirrored |= (ref.turn_boards(exp["own"], k) == exp["own"]) & (ref.turn_boards(exp["opp"], k) == exp["opp"])
    assert mirrored.any()


def test_canonical_rows_of_every_variant_of_every_row(rows):
    from iago_amd import ops
    own = np.concatenate([ref.turn_boards(rows["own"], k) for k in range(8)])
    opp = np.concatenate([ref.turn_boards(rows["opp"], k) for k in range(8)])
    c_own, c_opp, sym = ops.canonical_rows(ops.bits_to_tensor(own), ops.bits_to_tensor(opp))
    e_own, e_opp, e_sym = ref.canonical(own, opp)
    assert sym.dtype == torch.uint8
    assert np.array_equal(ops.tensor_to_bits(c_own), e_own) and np.array_equal(ops.tensor_to_bits(c_opp), e_opp)
    assert np.array_equal(sym.cpu().numpy(), e_sym)
    n = rows["own"].size
    assert np.array_equal(e_own.reshape(8, n), np.tile(e_own[:n], (8, 1)))   # one name for all eight
    assert set(e_sym.tolist()) == set(range(8))


def test_canonical_rows_of_edge_boards_and_the_start_position():
    from iago_amd import ops
    full = 0xFFFFFFFFFFFFFFFF
    own = np.array([0, full, full, 0, 0x00000000FFFFFFFF, START[0], START[1], 1, 1 << 63], dtype=np.uint64)
    opp = np.array([0, 0, 0, full, 0xFFFFFFFF00000000, START[1], START[0], 1 << 63, 1], dtype=np.uint64)
    c_own, c_opp, sym = ops.canonical_rows(ops.bits_to_tensor(own), ops.bits_to_tensor(opp))
    e_own, e_opp, e_sym = ref.canonical(own, opp)
    assert np.array_equal(ops.tensor_to_bits(c_own), e_own) and np.array_equal(ops.tensor_to_bits(c_opp), e_opp)
    assert np.array_equal(sym.cpu().numpy(), e_sym)
    # the start position: four variants tie for the smallest pair, the lowest of them is reported
    pairs = [(int(ref.turn_boards(own[5:6], k)[0]), int(ref.turn_boards(opp[5:6], k)[0])) for k in range(8)]
    assert sum(p == min(pairs) for p in pairs) == 4 and int(sym[5]) == pairs.index(min(pairs))
    assert sym[:4].tolist() == [0, 0, 0, 0]


def test_the_fixture_window_merges_to_the_restatement(merged_rows):
    w, got, exp = merged_rows
    assert (got.n_unique, got.count, got.total) == (exp["n_unique"], w.count, w.total)
    _same(got, exp, MERGED)
    assert int(got.mult.sum()) == w.count


def test_a_window_of_one_row(rows):
    w = _window({k: v[100:101] for k, v in rows.items()}, capacity=5)
    got, exp = w.merge(), ref.merge(*_host(w))
    assert got.n_unique == 1 == exp["n_unique"] and got.mult.tolist() == [1] and got.first.tolist() == [0]
    _same(got, exp, MERGED)


def test_a_ring_that_has_wrapped(rows):
    """Two adds into a ring smaller than their rows: slot order is not add order, and the oldest rows are gone."""
    from iago_amd.replay import ReplayWindow
    w = ReplayWindow(1000, seed=4)
    w.add(_tup(rows, 0, 700))
    w.add(_tup(rows, 700, 1400))
    assert w.total == 1400 > w.capacity == w.count
    assert int(w.cols["own"][0].item()) == int(rows["own"][1000].view(np.int64))   # (row 1000 lives in slot 0)
    got, exp = w.merge(), ref.merge(*_host(w))
    assert got.n_unique == exp["n_unique"] < 1000
    _same(got, exp, MERGED)


def _copies(rows, n, turn=20):
    """n rows that are one position -- a mid-game row without symmetry -- in variant j % 8, each with its own visit row
    (turned with its board) and result."""
    rs = np.random.RandomState(7 + turn)
    src = int(np.nonzero(rows["turn"] == turn)[0][0])
    pairs = {(int(ref.turn_boards(rows["own"][src:src + 1], k)[0]), int(ref.turn_boards(rows["opp"][src:src + 1], k)[0]))
             for k in range(8)}
    assert len(pairs) == 8
    base = np.where(rows["pi"][src] > 0, 1, 0) * rs.randint(0, 401, size=(n, 64))
    out = dict(own=np.zeros(n, np.uint64), opp=np.zeros(n, np.uint64), pi=np.zeros((n, 64), np.int32),
               z=rs.randint(-1, 2, size=n).astype(np.int8), turn=np.zeros(n, np.int64))
    for k in range(8):
        out["own"][k::8] = ref.turn_boards(rows["own"][src:src + 1], k)[0]
        out["opp"][k::8] = ref.turn_boards(rows["opp"][src:src + 1], k)[0]
        out["pi"][k::8] = ref.turn_rows(base[k::8].astype(np.int32), k)
    return out


def test_one_position_in_4096_copies_spread_over_its_symmetries(rows):
    w = _window(_copies(rows, 4096))
    got, exp = w.merge(), ref.merge(*_host(w))
    assert got.n_unique == 1 and got.mult.tolist() == [4096] == exp["mult"].tolist()
    _same(got, exp, MERGED)
    assert int(got.pi.sum()) == int(w.cols["pi"].sum())
    for mode in ("unique", "rows"):                                  # n_unique = 1: every draw is group 0
        s = w.sample(1000, step=2, merged=mode)
        assert bool((s["group"] == 0).all()) and set(s["sym"].tolist()) == set(range(8))
        _same(s, ref.sample(exp, w.count, w.seed, 2, 1000, mode), DRAWN)


def test_groups_on_both_sides_of_the_spread_threshold(rows):
    """A group of more than 512 rows is summed by several waves (one per 256 sorted rows), a smaller one by one wave:
    groups of 512, 513 and 700 rows and single rows, shuffled over the slots, so that the large groups start and end
    inside chunks and have small groups between them."""
    parts = [_copies(rows, 512, turn=18), _copies(rows, 513, turn=22), _copies(rows, 700, turn=26),
             {k: v[np.nonzero(rows["turn"] == 40)[0][:40]] for k, v in rows.items()}]
    r = {k: np.concatenate([p[k] for p in parts]) for k in ("own", "opp", "pi", "z")}
    shuffle = np.random.RandomState(3).permutation(r["own"].size)
    w = _window({k: v[shuffle] for k, v in r.items()})
    got, exp = w.merge(), ref.merge(*_host(w))
    assert sorted(exp["mult"].tolist())[-3:] == [512, 513, 700] and got.n_unique == exp["n_unique"] > 3
    _same(got, exp, MERGED)


def test_a_spread_group_clamps_and_flags_its_sums_too(rows):
    """600 rows of one position, 75 of them with 2^25 visits on one cell: 75 * 2^25 > 2^31 - 1, summed in 64 bits by
    three waves; the other cells stay exact."""
    from iago_amd import _lib, ops
    r = _copies(rows, 600, turn=24)
    cell = int(np.argmax(r["pi"][0]))
    r["pi"][0::8, cell] = 2 ** 25                                    # (variant 0's rows: the same canonical cell)
    w = _window(r)
    c = w.cols
    m = ops.replay_merge(c["own"], c["opp"], c["pi"], c["z"], 600)
    exp = ref.merge(*_host(w))
    assert exp["flags"] == ref.OVERFLOW and int(exp["pi"].max()) == 2 ** 31 - 1 and int((exp["pi"] == 2 ** 31 - 1).sum()) == 1
    assert m["meta"].tolist() == [1, _lib.REPLAY_MERGE_OVERFLOW]
    _same({k: m[k][:1] for k in MERGED}, exp, MERGED)


def _distinct(rows):
    c_own, c_opp, _ = ref.canonical(rows["own"], rows["opp"])
    keep = np.sort(np.unique(np.stack([c_own, c_opp], axis=1), axis=0, return_index=True)[1])
    return {k: v[keep] for k, v in rows.items()}


def test_a_window_without_duplicates(rows):
    d = _distinct(rows)
    w = _window(d)
    got, exp = w.merge(), ref.merge(*_host(w))
    assert got.n_unique == w.count == d["own"].size and bool((got.mult == 1).all())
    _same(got, exp, MERGED)
    assert got.first.tolist() == list(range(w.count))


def test_sums_beyond_int32_are_clamped_flagged_and_refused():
    from iago_amd import _lib, ops
    r = dict(own=np.full(3, START[0], np.uint64), opp=np.full(3, START[1], np.uint64), pi=np.zeros((3, 64), np.int32),
             z=np.ones(3, np.int8))
    r["pi"][:, 19] = 2 ** 30
    r["pi"][:, 26] = 2 ** 29
    w = _window(r)
    c = w.cols
    m = ops.replay_merge(c["own"], c["opp"], c["pi"], c["z"], 3)
    exp = ref.merge(*_host(w))
    assert exp["flags"] == ref.OVERFLOW == _lib.REPLAY_MERGE_OVERFLOW
    assert m["meta"].tolist() == [1, _lib.REPLAY_MERGE_OVERFLOW]
    _same({k: m[k][:1] for k in MERGED}, exp, MERGED)
    assert int(m["pi"][0].max()) == 2 ** 31 - 1
    with pytest.raises(_lib.IagoError, match="int32"):
        w.merge()
    with pytest.raises(_lib.IagoError, match="int32"):
        w.sample(4, merged="unique")
    two = ops.replay_merge(c["own"], c["opp"], c["pi"], c["z"], 2)   # 2^30 + 2^30 = 2^31 is already one too many
    assert two["meta"].tolist() == [1, _lib.REPLAY_MERGE_OVERFLOW]
    one = ops.replay_merge(c["own"], c["opp"], c["pi"], c["z"], 1)
    assert one["meta"].tolist() == [1, 0]


@pytest.mark.parametrize("step", [0, 5])
@pytest.mark.parametrize("mode", ["unique", "rows"])
def test_merged_draws_are_the_restatements(merged_rows, mode, step):
    w, m, exp = merged_rows
    got = w.sample(1000, step=step, merged=mode)
    assert set(got) == set(DRAWN)
    want = ref.sample(exp, w.count, w.seed, step, 1000, mode)
    _same(got, want, DRAWN)
    assert got["result"].dtype == torch.float32 and got["pi"].dtype == torch.int32
    assert len(set(got["group"].tolist())) > 300


def test_a_skewed_window_is_drawn_by_position_or_by_row(rows):
    """300 copies of the start position in front of 20 other positions: "rows" draws the start about 15 times in 16,
    "unique" about once in 21 -- and each is the restatement's draw."""
    d = _distinct(rows)
    far = np.nonzero(d["turn"] >= 30)[0][:20]
    r = {k: np.concatenate([np.repeat(v[:1], 300, axis=0), v[far]]) for k, v in d.items()}
    r["z"][:300] = np.random.RandomState(2).randint(-1, 2, size=300).astype(np.int8)
    w = _window(r, seed=9)
    got, exp = w.merge(), ref.merge(*_host(w))
    assert got.n_unique == 21 and int(got.mult.max()) == 300
    _same(got, exp, MERGED)
    start = int(np.argmax(exp["mult"]))
    share = {}
    for mode in ("unique", "rows"):
        s = w.sample(1000, step=1, merged=mode)
        _same(s, ref.sample(exp, w.count, w.seed, 1, 1000, mode), DRAWN)
        share[mode] = int((s["group"] == start).sum())
        mean = s["result"][s["group"] == start]
        assert bool((mean == float(np.float32(exp["z_sum"][start]) / np.float32(300))).all())
    assert share["rows"] > 850 and share["unique"] < 120


def test_an_add_after_a_merged_draw_rebuilds_the_snapshot(rows):
    from iago_amd.replay import ReplayWindow
    w = ReplayWindow(2000, seed=4)
    w.add(_tup(rows, 0, 600))
    a = w.sample(500, step=3, merged="unique")
    snap = w.merged()
    assert snap.total == 600 and w.merged() is snap                  # kept while nothing is added
    plain = w.sample(500, step=3)                                    # the unmerged draw neither needs nor drops it
    assert "move" in plain and w.merged() is snap
    w.add(_tup(rows, 600, 1500))
    b = w.sample(500, step=3, merged="unique")
    fresh = w.merged()
    assert fresh is not snap and (fresh.total, fresh.count) == (1500, 1500) and fresh.n_unique > snap.n_unique
    exp = ref.merge(*_host(w))
    _same(fresh, exp, MERGED)
    _same(b, ref.sample(exp, 1500, w.seed, 3, 500, "unique"), DRAWN)
    assert not torch.equal(a["group"], b["group"])
    assert w.step == 0
    w.sample(8, merged="rows")                                       # the window's own counter serves merged draws too
    assert w.step == 1


def test_step_from_window_merged_is_the_update_on_the_merged_draw(merged_rows):
    from iago_amd import network
    from iago_amd.train_rl import ReinforceTrainer
    w = merged_rows[0]
    torch.manual_seed(3)
    first = network.SLPolicy()
    twin = network.SLPolicy()
    twin.load_state_dict(first.state_dict())
    a = ReinforceTrainer(first, pool_dir=None, N=2, seed=1)
    b = ReinforceTrainer(twin, pool_dir=None, N=2, seed=1)
    before = w.step
    out = a.step_from_window(w, 256, merged="unique", step=6)
    assert set(out) == {"loss", "kl", "n_tuples", "step"} and out["n_tuples"] == 256 and out["step"] == 6
    assert np.isfinite(out["loss"]) and np.isfinite(out["kl"])
    s = w.sample(256, step=6, merged="unique")
    loss = b._update_visits(s["own"], s["opp"], s["pi"])
    assert float(loss.item()) == out["loss"]
    for (k, pa), pb in zip(a.model1.named_parameters(), b.model1.parameters()):
        assert torch.equal(pa, pb), k
    assert w.step == before and a.opt.t == 1
    with pytest.raises(ValueError, match="move"):
        a.step_from_window(w, 256, target="move", merged="rows")
