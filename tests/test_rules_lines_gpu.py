"""Every form of the rules on the device against the plain reference, bit for bit, on every content of every board line
(tests/line_cases.py: 131,166 positions bare and 131,166 with random stones off the line).

    A   8 lanes a board (othello_dev.hpp)        ops.legal_moves, ops.apply_moves, ops.play_turn; rollout hint 2
    B   a lane a board (othello_lane.hpp)        ops.alphabeta_moves(split=): the jobs are the children; ops.random_moves
    B'  the lane form with reversed boards       rollout hint 1
    C   16 lanes a board (rollout_row_body.hpp)  rollout hint 0 below 32768 boards, traced and as the production instance

The rollouts are held against orc.random_playout game for game: every bare case where either side can move, and every
ROLLOUT_NOISY_STRIDE-th noisy case.  The sampled Python references: 4096 roots of split 2, 512 roots of (score, move)."""
import time

import numpy as np
import pytest
import torch

from oracle import oracle as orc

from . import alphabeta_ref as ab
from . import alphabeta_split_ref as sr
from . import line_cases as lc
from .conftest import load_json
from .test_rollout_gpu import replay_check

pytestmark = pytest.mark.gpu

ROLLOUT_NOISY_STRIDE = 8
ROLLOUT_LAUNCH = 16384          # boards a rollout launch: below the 32768 at which hint 0 leaves the row kernel
ROLLOUT_SEED, ROLLOUT_ID_BASE = 31, 500000
SPLIT2_ROOTS, SPLIT2_PARTS = 2048, 4    # a variant; 4096 roots in all
SCORE_ROOTS = 256                        # a variant; 512 in all
MAXT = 128


@pytest.fixture(scope="module")
def ops():
    from iago_amd import ops as o
    assert torch.cuda.is_available(), "the -m gpu tests need a HIP device"
    return o


class Variant(object):
    def __init__(self, name):
        self.name = name
        self.own, self.opp, self.line_id = lc.cases(lc.VARIANTS[name])
        self.legal, self.flips = lc.reference_of(lc.VARIANTS[name])
        self.mobility = lc.popcount(self.legal)
        # the rows of the move kernels: (position, cell), the boards before and after
        self.pos, self.cell = lc.move_rows(self.own, self.opp, self.line_id, self.legal)
        self.row_flips = self.flips[self.pos, self.cell]
        self.child_own, self.child_opp = lc.children(self.own[self.pos], self.opp[self.pos], self.row_flips, self.cell)


@pytest.fixture(scope="module")
def variants():
    return {name: Variant(name) for name in lc.VARIANTS}


@pytest.fixture(scope="module", params=sorted(lc.VARIANTS))
def v(request, variants):
    return variants[request.param]


# ------------------------------------------------------------------------------------------------ form A
def test_legal_moves(ops, v):
    got = ops.tensor_to_bits(ops.legal_moves(ops.bits_to_tensor(v.own), ops.bits_to_tensor(v.opp)))
    bad = np.flatnonzero(got != v.legal)
    assert len(bad) == 0, (len(bad), int(bad[0]), hex(int(v.own[bad[0]])), hex(int(v.opp[bad[0]])))


def _first_bad(v, bad):
    i = int(bad[0])
    return len(bad), int(v.pos[i]), int(v.cell[i]), hex(int(v.own[v.pos[i]])), hex(int(v.opp[v.pos[i]]))


def test_apply_moves(ops, v):
    """Every empty cell of the line, legal or not (a ray that wraps shows as a flip there), and every legal move off it."""
    illegal = ((v.legal[v.pos] >> v.cell.astype(np.uint64)) & np.uint64(1)) == 0
    assert illegal.sum() > 200000 and not v.row_flips[illegal].any() and (~illegal).sum() == v.mobility.sum()
    o, p = ops.bits_to_tensor(v.own[v.pos]), ops.bits_to_tensor(v.opp[v.pos])
    ops.apply_moves(o, p, torch.from_numpy(v.cell.astype(np.int8)).cuda())
    bad = np.flatnonzero((ops.tensor_to_bits(o) != v.child_own) | (ops.tensor_to_bits(p) != v.child_opp))
    assert len(bad) == 0, _first_bad(v, bad)


def test_play_turn(ops, v):
    """The same rows through iago_play_turn: apply_moves' boards with the sides swapped, and the next mover's legal moves."""
    n, dev = len(v.pos), "cuda"
    o, p = ops.bits_to_tensor(v.own[v.pos]), ops.bits_to_tensor(v.opp[v.pos])
    active = torch.ones(n, dtype=torch.uint8, device=dev)
    stones = torch.zeros(n, dtype=torch.int32, device=dev)
    pass_flg, done = torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
    legal, active_next = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    ops.play_turn(o, p, torch.from_numpy(v.cell.astype(np.int8)).cuda(), active, stones, pass_flg, done, False, legal, active_next)
    bad = np.flatnonzero((ops.tensor_to_bits(o) != v.child_opp) | (ops.tensor_to_bits(p) != v.child_own))
    assert len(bad) == 0, _first_bad(v, bad)
    want = lc.reference_legal(v.child_opp, v.child_own)
    bad = np.flatnonzero(ops.tensor_to_bits(legal) != want)
    assert len(bad) == 0, _first_bad(v, bad)
    assert np.array_equal(active_next.cpu().numpy(), (want != 0).astype(np.uint8))
    assert bool((stones == 1).all()) and not bool(pass_flg.any()) and not bool(done.any())


# ------------------------------------------------------------------------------------------------ form B
def _np(r):
    torch.cuda.synchronize()
    return {k: (x.cpu().numpy() if isinstance(x, torch.Tensor) else x) for k, x in r.items()}


@pytest.fixture(scope="module")
def split1(ops, variants):
    """name -> ops.alphabeta_moves(depth=2, split=1) of all cases, launched once."""
    return {name: _np(ops.alphabeta_moves(ops.bits_to_tensor(x.own), ops.bits_to_tensor(x.opp), 2, split=1))
            for name, x in variants.items()}


def test_mobility_fits_the_split_table(variants):
    from iago_amd import engine
    assert max(int(x.mobility.max()) for x in variants.values()) <= engine.ALPHABETA_JOBS_PER_ROOT[1]
    assert int(variants["bare"].mobility.max()) == 3 and int(variants["noisy"].mobility.max()) >= 20


def test_split_1_jobs_are_the_children(v, split1):
    r = split1[v.name]
    n = lc.N_CASES
    assert not r["ctl"][[0, 2, 3, 6]].any() and r["done"].dtype == np.uint8 and (r["done"] == 1).all()
    count = np.maximum(1, v.mobility)
    assert np.array_equal(r["job_count"], count)
    first = np.cumsum(count) - count
    assert np.array_equal(r["job_first"], first)
    total = int(count.sum())
    assert r["jobs"] == total == len(r["job_own"]) and (r["job_done"] == 1).all()
    # the jobs wanted: a root that cannot move is its own job; every other root's legal moves ascending, each the child
    # from the child's mover's view
    pos, cell = lc.bits_of(v.legal)
    at = first[pos] + (np.arange(len(pos)) - (np.cumsum(v.mobility) - v.mobility)[pos])
    stuck = np.flatnonzero(v.mobility == 0)
    assert len(np.unique(np.concatenate([at, first[stuck]]))) == total
    c_own, c_opp = lc.children(v.own[pos], v.opp[pos], v.flips[pos, cell], cell)
    want_own, want_opp = np.empty(total, np.uint64), np.empty(total, np.uint64)
    want_root, want_path = np.empty(total, np.int64), np.zeros((total, 4), np.int64)
    want_own[at], want_opp[at], want_root[at] = c_opp, c_own, pos
    want_path[at] = np.stack([np.full(len(pos), 1), cell, np.full(len(pos), -1), np.zeros(len(pos), np.int64)], axis=1)
    want_own[first[stuck]], want_opp[first[stuck]], want_root[first[stuck]] = v.own[stuck], v.opp[stuck], stuck
    want_path[first[stuck]] = [2, -1, -1, 0]
    assert n == len(count) and len(stuck) == (2 if v.name == "noisy" else 65286)
    for k, want in (("job_root", want_root), ("job_path", want_path)):
        bad = np.flatnonzero((r[k] != want).reshape(total, -1).any(axis=1))
        assert len(bad) == 0, (k, len(bad), int(bad[0]), int(want_root[bad[0]]))
    for k, want in (("job_own", want_own), ("job_opp", want_opp)):
        bad = np.flatnonzero(r[k].view(np.uint64) != want)
        assert len(bad) == 0, (k, len(bad), int(bad[0]), int(want_root[bad[0]]), want_path[bad[0]].tolist())


def _sample(count):
    idx = (np.arange(count, dtype=np.int64) * lc.N_CASES) // count
    assert len(np.unique(idx)) == count
    return idx


@pytest.fixture(scope="module")
def split2(ops, variants):
    """name -> (the sampled roots, ops.alphabeta_moves(depth=3, split=2) of them), launched once."""
    idx = _sample(SPLIT2_ROOTS)
    return {name: (idx, _np(ops.alphabeta_moves(ops.bits_to_tensor(x.own[idx]), ops.bits_to_tensor(x.opp[idx]), 3, split=2)))
            for name, x in variants.items()}


@pytest.mark.parametrize("part", range(SPLIT2_PARTS))
def test_split_2_jobs_are_the_restatements(v, split2, part):
    idx, r = split2[v.name]
    assert not r["ctl"][[0, 2, 3, 6]].any() and (r["done"] == 1).all() and (r["job_done"] == 1).all()
    per = SPLIT2_ROOTS // SPLIT2_PARTS
    kinds = np.zeros(3, dtype=np.int64)
    for s in range(part * per, (part + 1) * per):
        want = sr.jobs_of(v.own[idx[s]], v.opp[idx[s]], 3, 2)
        kinds += sr.job_kinds(want)
        lo = int(r["job_first"][s])
        assert r["job_count"][s] == len(want), s
        got = [(int(np.uint64(r["job_own"][j])), int(np.uint64(r["job_opp"][j]))) + tuple(int(x) for x in r["job_path"][j, :3])
               for j in range(lo, lo + len(want))]
        assert got == want and (r["job_root"][lo:lo + len(want)] == s).all(), (s, int(idx[s]))
        assert not r["job_path"][lo:lo + len(want), 3].any()
    # roots that are their own job, children that cannot move, and whole two-ply jobs are all in every part
    assert kinds[2] > 0 and (v.name == "noisy" or (kinds[0] > 100 and kinds[1] > 100)), kinds


def test_scores_and_moves_of_sampled_roots(v, split1):
    r = split1[v.name]
    idx = _sample(SCORE_ROOTS)
    want = [ab.alphabeta(v.own[i], v.opp[i], 2) for i in idx]
    assert list(zip(r["score"][idx].tolist(), r["move"][idx].tolist())) == want
    if v.name == "bare":
        assert {-1, -2} <= {m for _, m in want}


def test_random_moves(ops, v):
    seed, id_base, id_mod, turn = 77, 1000, 8192, 5
    got = ops.random_moves(ops.bits_to_tensor(v.own), ops.bits_to_tensor(v.opp), seed, id_base, id_mod, turn).cpu().numpy()
    assert np.array_equal(got == -1, v.legal == 0)
    word = np.array([ab.word(seed, ab.opening_id(g, id_base, id_mod), turn) for g in range(id_mod)], dtype=np.uint64)
    w = word[np.arange(lc.N_CASES) % id_mod]
    assert ab.random_index(int(w[9000]), 7) == int((w[9000] * np.uint64(7)) >> np.uint64(32))
    r = ((w * v.mobility.astype(np.uint64)) >> np.uint64(32)).astype(np.int64)      # (32 bits x at most 64: no overflow)
    want = lc.nth_bit(v.legal, r)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (len(bad), int(bad[0]))
    if v.name == "noisy":
        assert len(np.unique(r)) >= 15         # low and high ranks drawn alike


# ------------------------------------------------------------------------------------------------ whole playouts
class Playouts(object):
    """The oracle's uniform playouts of a variant's rollout cases, computed once for all three hints."""

    def __init__(self, x):
        if x.name == "bare":
            keep = np.flatnonzero((x.legal != 0) | (lc.reference_legal(x.opp, x.own) != 0))
            assert len(keep) == 96676
        else:
            keep = np.arange(0, lc.N_CASES, ROLLOUT_NOISY_STRIDE)
        self.own, self.opp = x.own[keep], x.opp[keep]
        n = len(keep)
        states = lc.states_of(self.own, self.opp)
        self.trace = np.full((MAXT, n), 0xFE, dtype=np.uint8)
        self.z, self.n_turns = np.empty(n, np.int8), np.empty(n, np.uint8)
        finals = np.empty((n, 8, 8), np.float32)
        t0 = time.time()
        for b in range(n):
            self.z[b], finals[b], tr = orc.random_playout(states[b], 1, ROLLOUT_SEED, game_id=ROLLOUT_ID_BASE + b)
            self.n_turns[b] = len(tr)
            self.trace[:len(tr), b] = np.array(tr, dtype=np.int64) & 0xFF      # (-1, a pass, is 0xFF)
        self.seconds = time.time() - t0
        self.final_own, self.final_opp = lc.boards_of(finals)
        print("oracle playouts, %s: %d games, %.1f s, %d turns at most" % (x.name, n, self.seconds, self.n_turns.max()))


@pytest.fixture(scope="module")
def playouts(variants):
    return {name: Playouts(x) for name, x in variants.items()}


def _rollout(ops, own, opp, hint, trace=True, weights=None, seed=ROLLOUT_SEED, id_base=ROLLOUT_ID_BASE):
    """ops.rollout in launches of ROLLOUT_LAUNCH boards: (z, final_own, final_opp, n_turns, trace)."""
    out = []
    for lo in range(0, len(own), ROLLOUT_LAUNCH):
        o, p = ops.bits_to_tensor(own[lo:lo + ROLLOUT_LAUNCH]), ops.bits_to_tensor(opp[lo:lo + ROLLOUT_LAUNCH])
        assert o.numel() < 32768
        res = ops.rollout(o, p, weights, seed=seed, id_base=id_base + lo, want_final=True, want_turns=True, want_trace=trace,
                          throughput_hint=hint)
        torch.cuda.synchronize()
        assert (res.trace is not None) == trace
        out.append((res.z.cpu().numpy(), ops.tensor_to_bits(res.final_own), ops.tensor_to_bits(res.final_opp),
                    res.n_turns.cpu().numpy(), res.trace.cpu().numpy() if trace else np.zeros((MAXT, o.numel()), np.uint8)))
    return tuple(np.concatenate([part[k] for part in out], axis=-1) for k in range(5))


@pytest.mark.parametrize("hint", [0, 1, 2])
def test_uniform_playouts_are_the_oracles(ops, v, playouts, hint):
    want = playouts[v.name]
    z, fo, fp, nt, tr = _rollout(ops, want.own, want.opp, hint)
    for name, got, ref in (("n_turns", nt, want.n_turns), ("z", z, want.z), ("final_own", fo, want.final_own),
                           ("final_opp", fp, want.final_opp), ("trace", tr, want.trace)):
        bad = np.flatnonzero((got != ref).reshape(-1, len(z)).any(axis=0))
        assert len(bad) == 0, (name, len(bad), int(bad[0]), hex(int(want.own[bad[0]])), hex(int(want.opp[bad[0]])))


def test_production_row_kernel_plays_the_traced_games(ops, v, playouts):
    want = playouts[v.name]
    z, fo, fp, nt, _ = _rollout(ops, want.own, want.opp, 0, trace=False)
    assert np.array_equal(z, want.z) and np.array_equal(nt, want.n_turns)
    assert np.array_equal(fo, want.final_own) and np.array_equal(fp, want.final_opp)


# ------------------------------------------------------------------------------------------------ the rollout policy
@pytest.mark.parametrize("hint", [0, 1, 2])
def test_policy_rollout_on_row_contents(ops, variants, hint):
    """The row kernel looks its policy factors up by windows of a board row: 64 contents of each of the 8 rows, noisy."""
    x = variants["noisy"]
    first = lc.line_first()
    idx = np.concatenate([first[row] + (np.arange(64) * 3 ** 8) // 64 for row in range(8)])
    assert len(idx) == 512 and (x.line_id[idx] == np.repeat(np.arange(8), 64)).all()
    g = load_json("simulate.json")
    w, bvec = g["w"], g["b"]
    seed, id_base = 11, 77
    own, opp = x.own[idx], x.opp[idx]
    out = _rollout(ops, own, opp, hint, weights=ops.RolloutWeights(w, bvec), seed=seed, id_base=id_base)
    sampled, exact = replay_check(own, opp, *out, w, bvec, lambda b, t: orc.uniform(seed, id_base + b, t, 0))
    print("policy rollout on row contents, hint %d: sampled %d, exact %d" % (hint, sampled, exact))
    assert sampled > 5000
    assert sampled - exact <= -(-3 * sampled // 10000), (sampled, exact)
