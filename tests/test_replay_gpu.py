"""The replay window on the GPU (iago_replay_sample, ops.replay_sample / augment8_visits, replay.ReplayWindow, the
trainers' entry points on it): the kernel's draw and its eight symmetries against tests/replay_ref.py bit for bit,
properties that need no reference (the transformed visit rows lie on the transformed board's legal moves), rows that
fail the device's check, and the updates fed from a window against the same updates fed by hand.  The rows are those
of ONE small exploring self-play (8 games, 8 playouts) behind a few hand-made ones."""
import numpy as np
import pytest
import torch

from tests import replay_ref
from tests.conftest import load_json

pytestmark = pytest.mark.gpu

COLS = ("own", "opp", "pi", "move", "z")
HAND = 6   # hand-made rows in front of the searched ones


@pytest.fixture(scope="module")
def played():
    """(the policy the search used, the value net, the round's tuples)."""
    from iago_amd import engine, network, ops
    torch.manual_seed(3)
    policy = network.SLPolicy().cuda().eval()
    value = network.Value().cuda().eval()
    g = load_json("simulate.json")
    # (n_thr = 2: with 8 playouts a root must expand early to have children and visits at all)
    m = engine.BatchedMCTS(8, policy, value, ops.RolloutWeights(g["shipped_w"], g["shipped_b"]), n_thr=2,
                           capacity=4096, seed=11, persistent=True)
    tup = {k: v.clone() for k, v in engine.SelfPlayEngine(m).play(8, explore_turns=8).tuples().items()}
    m.close()
    assert tup["own"].numel() >= 300 - HAND                      # (8 games of about 60 searched turns)
    return policy, value, tup


@pytest.fixture(scope="module")
def rows(played):
    """300 window rows on the device and as numpy: HAND hand-made ones -- a visit row with a single count in each
    corner, move -1, every z -- then searched ones."""
    from iago_amd import ops
    tup = played[2]
    n = 300 - HAND
    pi = torch.zeros((HAND, 64), dtype=torch.int32)
    for r, cell in enumerate((0, 7, 56, 63)):
        pi[r, cell] = 5 + r
    pi[4] = torch.arange(64, dtype=torch.int32)
    hand = dict(own=ops.bits_to_tensor([1, 1 << 7, 1 << 56, 1 << 63, 0x0000001008000000, 0], "cpu"),
                opp=ops.bits_to_tensor([0x8000000000000000, 2, 4, 8, 0x0000000810000000, 0xFFFFFFFFFFFFFFFF], "cpu"),
                pi=pi, move=torch.tensor([0, 7, -1, 63, 19, -1], dtype=torch.int8),
                z=torch.tensor([-1, 0, 1, 1, -1, 0], dtype=torch.int8))
    dev = {k: torch.cat([hand[k].cuda(), tup[k][:n].to(hand[k].dtype)]).contiguous() for k in COLS}
    host = {k: v.cpu().numpy() for k, v in dev.items()}
    return dev, host


def _window(rows, capacity):
    return {k: v[:capacity].contiguous() for k, v in rows[0].items()}


def _permute_bits(x, m):
    """uint64 boards with bit m[a] set where x has bit a set."""
    cells = np.arange(64, dtype=np.uint64)
    on = (x.reshape(-1, 1) >> cells) & np.uint64(1)
    out = np.zeros_like(on)
    out[:, m] = on
    return np.bitwise_or.reduce(out << cells, axis=1)


def _expected(host, slot, sym):
    """The kernel's outputs for the given slots and variants, on replay_ref.cell_map."""
    n = len(slot)
    exp = dict(own=np.zeros(n, np.uint64), opp=np.zeros(n, np.uint64), pi=np.zeros((n, 64), np.int32),
               move=np.zeros(n, np.int8), z=host["z"][slot].copy(), slot=slot.astype(np.int32), sym=sym.astype(np.uint8))
    for k in range(8):
        at = np.nonzero(sym == k)[0]
        if not at.size:
            continue
        m = np.array(replay_ref.cell_map(k))
        src = slot[at]
        exp["own"][at] = _permute_bits(host["own"][src].view(np.uint64), m)
        exp["opp"][at] = _permute_bits(host["opp"][src].view(np.uint64), m)
        row = np.zeros((at.size, 64), np.int32)
        row[:, m] = host["pi"][src]
        exp["pi"][at] = row
        mv = host["move"][src].astype(np.int64)
        exp["move"][at] = np.where(mv < 0, mv, m[np.maximum(mv, 0)]).astype(np.int8)
    exp["result"] = exp["z"].astype(np.float32)
    return exp


def _same(got, exp):
    for k, want in exp.items():
        have = got[k].cpu().numpy()
        if k in ("own", "opp"):
            have = have.view(np.uint64)
        assert have.dtype == want.dtype and np.array_equal(have, want), k


def test_the_vector_reference_is_replay_ref_apply(rows):
    """_expected (whole batches at once) against replay_ref.apply row by row: every variant of the first 40 rows."""
    host = rows[1]
    slot, sym = np.repeat(np.arange(40), 8), np.tile(np.arange(8), 40)
    exp = _expected(host, slot, sym)
    for j in range(slot.size):
        s = slot[j]
        o, p, pi, mv = replay_ref.apply(host["own"].view(np.uint64)[s], host["opp"].view(np.uint64)[s], host["pi"][s],
                                        host["move"][s], sym[j])
        assert (int(exp["own"][j]), int(exp["opp"][j]), int(exp["move"][j])) == (o, p, mv)
        assert np.array_equal(exp["pi"][j], pi)


SHAPES = [(8, 1, 1), (8, 3, 64), (8, 8, 65), (8, 3, 4096), (300, 257, 4096)]


@pytest.mark.parametrize("step", [0, 1, 2 ** 32 - 1])
@pytest.mark.parametrize("seed", [0, 0x9E3779B97F4A7C15])
@pytest.mark.parametrize("capacity,count,n", SHAPES)
def test_drawn_rows_are_the_references(rows, capacity, count, n, seed, step):
    from iago_amd import ops
    w = _window(rows, capacity)
    got = ops.replay_sample(w["own"], w["opp"], w["pi"], w["move"], w["z"], count, n=n, seed=seed, step=step)
    draws = np.array([replay_ref.draw(seed, step, j, count) for j in range(n)], dtype=np.int64)
    slot, sym = draws[:, 0], draws[:, 1]
    assert slot.min() >= 0 and slot.max() < count
    _same(got, _expected(rows[1], slot, sym))
    if n == 4096 and count == 3:
        assert set(slot.tolist()) == {0, 1, 2} and set(sym.tolist()) == set(range(8))
        assert set(got["slot"].tolist()) == {0, 1, 2} and set(got["sym"].tolist()) == set(range(8))


def test_given_slots_and_variants_are_taken(rows):
    from iago_amd import ops
    w = _window(rows, 300)
    rs = np.random.RandomState(8)
    slot = np.concatenate([np.repeat(np.arange(HAND), 8), rs.randint(0, 257, size=700)])
    sym = np.concatenate([np.tile(np.arange(8), HAND), rs.randint(0, 8, size=700)])
    flags = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = ops.replay_sample(w["own"], w["opp"], w["pi"], w["move"], w["z"], 257,
                            slot=torch.from_numpy(slot.astype(np.int32)).cuda(),
                            sym=torch.from_numpy(sym.astype(np.uint8)).cuda(), flags=flags)
    _same(got, _expected(rows[1], slot, sym))
    assert int(flags.item()) == 0
    with pytest.raises(ValueError, match="both or neither"):
        ops.replay_sample(w["own"], w["opp"], w["pi"], w["move"], w["z"], 257, n=4, slot=got["slot"][:4])
    with pytest.raises(TypeError):
        ops.replay_sample(w["own"], w["opp"], w["pi"].to(torch.int64), w["move"], w["z"], 257, n=4)
    with pytest.raises(ValueError, match="contiguous"):
        ops.replay_sample(w["own"], w["opp"], w["pi"], w["move"], torch.zeros(600, dtype=torch.int8, device="cuda")[::2], 257, n=4)


def test_augment8_visits_is_augment8_with_the_visit_rows(rows):
    from iago_amd import ops
    dev, host = rows
    n = 77
    own, opp, act, pi = (dev[k][:n].contiguous() for k in ("own", "opp", "move", "pi"))
    oo, po, ao = ops.augment8(own, opp, act)
    o8, p8, a8, pi8 = ops.augment8_visits(own, opp, act, pi)
    assert torch.equal(o8, oo) and torch.equal(p8, po) and torch.equal(a8, ao)
    assert pi8.shape == (8, n, 64) and pi8.dtype == torch.int32
    exp = _expected(host, np.tile(np.arange(n), 8), np.repeat(np.arange(8), n))
    assert np.array_equal(pi8.cpu().numpy().reshape(-1, 64), exp["pi"])


def test_visit_rows_stay_on_the_legal_moves_and_keep_their_counts(rows):
    """No reference: a searched row's visits lie on its position's legal moves, so the transformed row lies on the
    transformed position's (ops.legal_moves); the counts and the stones are only moved."""
    from iago_amd import ops
    dev = rows[0]
    w = _window(rows, 300)
    got = ops.replay_sample(w["own"], w["opp"], w["pi"], w["move"], w["z"], 300, n=2048, seed=5, step=9)
    real = got["slot"] >= HAND
    assert int(real.sum()) > 1900
    legal = ops.legal_moves(got["own"], got["opp"])
    on = ((legal.reshape(-1, 1) >> torch.arange(64, device="cuda")) & 1).to(torch.bool)
    assert bool((~(got["pi"] > 0) | on)[real].all())
    assert bool((got["pi"][real] > 0).any())                     # (not vacuous: searched rows carry visits)
    src = got["slot"].to(torch.int64)
    assert torch.equal(got["pi"].sum(dim=1), dev["pi"][src].sum(dim=1))

    def popcount(x):
        return ((x.reshape(-1, 1) >> torch.arange(64, device="cuda")) & 1).sum(dim=1)
    assert torch.equal(popcount(got["own"]), popcount(dev["own"][src]))
    assert torch.equal(popcount(got["opp"]), popcount(dev["opp"][src]))


def test_slots_and_variants_out_of_range_read_nothing(rows):
    """Slots count and -1 and variant 8: the rows come back as zeros with move -1 and bit 0 of flags, their neighbours
    are right.  (The kernel checks before it reads: nothing here is out of range on the device.)"""
    from iago_amd import ops
    count = 257
    w = _window(rows, 300)
    slot = np.array([0, count, 1, -1, 2, 5, 256], dtype=np.int32)
    sym = np.array([1, 0, 8, 3, 5, 255, 7], dtype=np.uint8)
    bad = np.array([False, True, True, True, False, True, False])
    flags = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = ops.replay_sample(w["own"], w["opp"], w["pi"], w["move"], w["z"], count,
                            slot=torch.from_numpy(slot).cuda(), sym=torch.from_numpy(sym).cuda(), flags=flags)
    assert int(flags.item()) & 1
    exp = _expected(rows[1], np.where(bad, 0, slot), np.where(bad, 0, sym))
    for k in ("own", "opp", "pi", "z", "result"):
        exp[k][bad] = 0
    exp["move"][bad] = -1
    exp["slot"], exp["sym"] = slot, sym                          # (repeated as supplied)
    _same(got, exp)


def _filled(rows, capacity=300, seed=4):
    from iago_amd.replay import ReplayWindow
    w = ReplayWindow(capacity, seed=seed)
    w.add(rows[0])
    return w


def test_the_window_draws_the_same_rows_for_the_same_step(rows):
    from iago_amd import _lib
    w = _filled(rows)
    a, b, c = w.sample(500, step=6), w.sample(500, step=6), w.sample(500, step=7)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["slot"], c["slot"]) and not torch.equal(a["sym"], c["sym"])
    assert w.step == 0
    first, second = w.sample(500), w.sample(500)
    assert w.step == 2
    zero, one = w.sample(500, step=0), w.sample(500, step=1)
    assert all(torch.equal(first[k], zero[k]) and torch.equal(second[k], one[k]) for k in first)
    assert not torch.equal(first["slot"], second["slot"])
    other = _filled(rows, seed=5).sample(500, step=0)
    assert not torch.equal(first["slot"], other["slot"])
    draws = [replay_ref.draw(4, 0, j, 300) for j in range(500)]
    assert first["slot"].tolist() == [d[0] for d in draws] and first["sym"].tolist() == [d[1] for d in draws]
    g = w.gather([3, 299, 0], 2)
    _same(g, _expected(rows[1], np.array([3, 299, 0]), np.array([2, 2, 2])))
    with pytest.raises(_lib.IagoError, match="outside"):
        w.gather([3, 300], 0)
    again = w.sample(500, step=0)                                # (the flag was cleared with the error)
    assert all(torch.equal(first[k], again[k]) for k in first)


def _policy_trainer(policy):
    """A trainer on a fresh module with the policy's parameters (a module the search has used holds ctypes templates
    of its weights, which do not deep-copy)."""
    from iago_amd import network
    from iago_amd.train_rl import ReinforceTrainer
    model = network.SLPolicy()
    model.load_state_dict(policy.state_dict())
    return ReinforceTrainer(model, pool_dir=None, N=2, seed=1)


def test_add_to_window_holds_the_canonical_rows_of_step_from_tuples(played, monkeypatch):
    from iago_amd.replay import ReplayWindow
    policy, _, tup = played
    tr = _policy_trainer(policy)
    seen = {}
    monkeypatch.setattr(tr, "_update_visits", lambda own, opp, pi: seen.update(own=own, opp=opp, pi=pi) or
                        torch.zeros((), device="cuda"))
    tr.step_from_tuples(tup, target="visits")
    n = tup["own"].numel()
    w = ReplayWindow(n + 10, seed=1)
    assert tr.add_to_window(w, tup) == n and (w.count, w.total) == (n, n)
    g = w.gather(torch.arange(n), 0)
    assert torch.equal(g["own"], seen["own"]) and torch.equal(g["opp"], seen["opp"]) and torch.equal(g["pi"], seen["pi"])
    order = torch.argsort(tup["turn"].to(torch.int64) * (1 << 32) + tup["game"].to(torch.int64), stable=True)
    for k in COLS:
        assert torch.equal(g[k], tup[k][order].to(g[k].dtype)), k
    assert torch.equal(g["result"], tup["z"][order].to(torch.float32))
    assert bool((g["sym"] == 0).all()) and g["slot"].tolist() == list(range(n))
    black = int((tup["colour"] == 1).sum())
    w1 = ReplayWindow(n, seed=1)
    assert tr.add_to_window(w1, tup, colour=1) == black == w1.count


def test_step_from_window_is_the_update_on_the_sampled_rows(played):
    from iago_amd.replay import ReplayWindow
    policy, _, tup = played
    a, b = _policy_trainer(policy), _policy_trainer(policy)
    w = ReplayWindow(1024, seed=9)
    a.add_to_window(w, tup)
    out = a.step_from_window(w, 256, target="visits", step=5)
    assert set(out) == {"loss", "kl", "n_tuples", "step"} and out["n_tuples"] == 256 and out["step"] == 5
    assert np.isfinite(out["loss"]) and np.isfinite(out["kl"]) and out["kl"] >= -1e-5
    rows = w.sample(256, step=5)
    loss = b._update_visits(rows["own"], rows["opp"], rows["pi"])
    assert float(loss.item()) == out["loss"]
    for (k, pa), pb in zip(a.model1.named_parameters(), b.model1.parameters()):
        assert torch.equal(pa, pb), k
    assert a.opt.t == 1 and w.step == 0
    nxt = a.step_from_window(w, 256)                             # the window's own counter
    assert nxt["step"] == 0 and w.step == 1 and a.opt.t == 2
    mv = a.step_from_window(w, 256, target="move")
    assert np.isfinite(mv["loss"]) and "kl" not in mv and mv["step"] == 1 and a.opt.t == 3
    with pytest.raises(ValueError, match="target"):
        a.step_from_window(w, 256, target="bogus")


def test_step_rows_is_value_grads_and_adam_on_the_sampled_results(played, rows):
    from iago_amd import network
    from iago_amd.train_rl import ChainerAdam
    from iago_amd.train_supervised import DROPOUT_RATIO, SupervisedTrainer
    value = played[1]
    s = _filled(rows).sample(256, step=3)
    models = []
    for _ in range(2):
        m = network.Value()
        m.load_state_dict(value.state_dict())
        models.append(m.cuda())
    tr = SupervisedTrainer(models[0], "value", seed=21, native=True)
    loss = tr.step_rows(s["own"], s["opp"], s["result"])
    assert np.isfinite(loss) and tr.opt.t == 1
    twin = models[1].train()
    gen = torch.Generator(device="cuda").manual_seed(21)
    keep = torch.rand((256, 128), device="cuda", generator=gen) >= DROPOUT_RATIO
    loss2 = twin.value_grads(s["own"], s["opp"], s["result"], keep=keep)
    twin.check_saturation()
    ChainerAdam(twin).update()
    assert float(loss2.item()) == loss
    for (k, pa), pb in zip(tr.model.named_parameters(), twin.parameters()):
        assert torch.equal(pa, pb), k
