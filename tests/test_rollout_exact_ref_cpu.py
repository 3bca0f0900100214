"""Guards of the exact rollout reference (tests/rollout_exact_ref.py), no GPU: that it states the oracle's policy and
rules, that the probes of tests/test_rollout_exact_gpu.py read every table entry a legal cell can read, that a
wrongly indexed table would move their draws, that few turns have to be refused, and that the extreme-uniform test
reaches the 16-lane kernel's fix-up branch."""
import os

import numpy as np
import pytest

from oracle import oracle as orc
from tests import rollout_exact_ref as R

RICH = ["rich%d" % s for s in R.RICH_SEEDS]
ALL_SETS = [s[0] for s in R.weight_sets()]


def test_weight_sets_are_what_they_say():
    sets = R.weight_sets()
    assert len(sets) == 18 + 1 + 3 and len(set(ALL_SETS)) == 22
    for name, kw, kb in sets[:18]:
        assert np.count_nonzero(kw) == 1 and kw.sum() == 2 and not kb.any()
    assert len({tuple(kw.reshape(-1)) for _, kw, _ in sets[:18]}) == 18
    assert not sets[18][1].any() and sets[18][2].tolist() == [(7 * c) % 4 for c in range(64)]
    for name, kw, kb in sets[19:]:
        assert np.all(kw != 0) and np.abs(kw).max() == 2 and kb.min() == 0 and kb.max() == 3


def test_rules_equal_the_oracle():
    """legal_moves / flips on synthetic probes, and play()'s turn structure: under the all-zero weight set the exact
    rule is floor(u n) in float32, which is orc.random_playout's draw -- whole games, passes, ends and z."""
    own, opp = R.probes(300, seed=3)
    legal = R.legal_moves(own, opp)
    for i in range(len(own)):
        s = orc.bits_to_state(int(own[i]), int(opp[i]))
        acts = orc.legal_actions(s, 1)
        assert orc.actions_to_mask(acts) == int(legal[i]), i
        for a in acts[:4]:
            s2 = s.copy()
            orc.place_stone(s2, a, 1)
            f = int(R.flips(own[i:i + 1], opp[i:i + 1], np.array([a]))[0])
            assert orc.state_to_bits(s2) == (int(own[i]) | f | (1 << a), int(opp[i]) & ~f), (i, a)
    edge = np.load(os.path.join(os.path.dirname(__file__), "golden", "rules.npz"))["edge_boards"]
    po, pp = R.positions_by_play(40, seed=2, n_start=10)
    own = np.concatenate([edge[:, 0], edge[:, 1], po, np.array([0xFFFFFFFFFFFFFFFF], np.uint64)])
    opp = np.concatenate([edge[:, 1], edge[:, 0], pp, np.array([0], np.uint64)])
    assert own.dtype == np.uint64 and opp.dtype == np.uint64
    games = R.exact_game(own, opp, np.zeros((2, 3, 3), int), np.zeros(64, int), R.philox_uniforms(9, 5, 2))
    assert games.kept.all()
    for b in range(len(own)):
        z, final, tr = orc.random_playout(orc.bits_to_state(int(own[b]), int(opp[b])), 1, seed=9, game_id=5 + b, stream=2)
        nt = int(games.n_turns[b])
        assert [(-1 if a == R.PASS else int(a)) for a in games.trace[:nt, b]] == tr, b
        assert np.all(games.trace[nt:, b] == R.UNWRITTEN)
        assert (int(games.final_own[b]), int(games.final_opp[b])) == orc.state_to_bits(final) and games.z[b] == z, b


@pytest.mark.parametrize("name", RICH)
def test_reference_states_the_oracles_policy(name):
    """Guard 1: on 200 probes the integer probabilities 2^K / sum are the float oracle's to 1e-5, and away from the
    CDF's boundaries the integer draw is orc.choice_cdf's."""
    _, kw, kb = R.set_by_name(name)
    w, b = R.float_weights(kw, kb)
    own, opp = R.probes(200, seed=2)
    u = (np.random.RandomState(4).randint(0, 1 << 24, 200) * R.GRID).astype(np.float32)
    K = R.exponents(own, opp, kw, kb)
    cells = R.draw(own, opp, kw, kb, u)
    away = 0
    for i, acts, p in R.oracle_probs(own, opp, w, b):
        mine = np.zeros(64)
        mine[acts] = 2.0 ** (K[i, acts] - K[i, acts].max())
        mine /= mine.sum()
        assert np.max(np.abs(mine - p)) < 1e-5, i
        if not R.near_boundary(p, acts, u[i]):
            away += 1
            assert cells[i] == orc.choice_cdf(p, float(u[i])), i
    assert away >= 190


@pytest.mark.parametrize("name", ALL_SETS)
def test_built_tables_snap_to_powers_of_two(name):
    """iago_rollout_build_table (host code) on the integer weight sets: product form, and every entry within 1e-3 of
    the power of two it is snapped to (snapped_weights asserts both)."""
    from iago_amd import ops
    _, kw, kb = R.set_by_name(name)
    table = R.snapped_weights(ops, kw, kb, device="cpu").table.numpy()
    assert np.all(np.log2(np.delete(table, np.arange(len(table) - 1028, len(table) - 1024))) % 1.0 == 0)


def test_not_order_free_is_refused():
    _, kw, kb = R.set_by_name("rich0")
    own, opp = R.probes(50)
    with pytest.raises(R.NotOrderFree):
        R.draw(own, opp, 13 * kw, kb, np.zeros(50, np.float32))
    assert not R.order_free(own, opp, 13 * kw, kb).all()


@pytest.mark.parametrize("name", ALL_SETS)
def test_probes_read_every_table_entry(name):
    """Guard 2, for every weight set (the one-tap and bias sets run on the same 4,099 probes as the rich ones): over
    the kept probes of the one-turn test, every entry a legal cell CAN read is read.  What cannot
    be (R.reachable): a legal cell is empty, so for ky = 1 the 16 windows / 16 row bytes per half whose four
    cells are all occupied feed none; it has an opponent stone beside it, so the empty opponent neighbourhood and the
    full own neighbourhood occur at none.  752 of 768 window entries, 255 of 256 centre-empty neighbourhoods per
    plane, every row byte for ky = 0, 2 and every byte with a zero bit in the cell's half for ky = 1."""
    case = R.one_turn_case(name)
    t4, nbh, rowb = R.coverage(case.own, case.opp)
    rt4, rnbh, rrowb = R.reachable()
    assert rt4.sum() == 752 and rnbh.sum(axis=1).tolist() == [255, 255]
    assert rrowb[[0, 2]].all() and rrowb[1].sum() == 2 * 2 * 240
    assert np.array_equal(t4, rt4), (int(t4.sum()), np.argwhere(t4 != rt4)[:5])
    assert np.array_equal(nbh, rnbh), (nbh.sum(axis=1), np.argwhere(nbh != rnbh)[:5])
    assert np.array_equal(rowb, rrowb), (int(rowb.sum()), np.argwhere(rowb != rrowb)[:5])


def test_probe_count_is_the_smallest_that_covers():
    own, opp = R.probes(R.N_PROBES)
    half = (R.N_PROBES - 3) // 2 + 3
    got, want = R.coverage(own[:half], opp[:half]), R.reachable()
    assert not all(np.array_equal(g, w) for g, w in zip(got, want))
    for n in (R.N_PROBES, R.PHILOX_N, R.EXTREME_N, R.BOUNDARY_N):
        assert n % 16 and n % 32 and n % 256      # a ragged tail in every kernel
    assert not np.any(own & opp) and np.all(R.legal_moves(own, opp) != 0)


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_mutated_reference_disagrees(mutation):
    """Guard 3: a reference with that indexing mistake draws another cell on at least 20 probes of the one-turn
    data of every rich set (and of the bias set, for the bias's own)."""
    for name in RICH + (["bias"] if mutation == "bias_mirror" else []):
        _, kw, kb = R.set_by_name(name)
        case = R.one_turn_case(name)
        wrong = R.draw(case.own, case.opp, kw, kb, case.u, mutation=mutation, strict=False)
        assert int((wrong != case.cell).sum()) >= 20, (name, mutation)


@pytest.mark.parametrize("name", ALL_SETS)
def test_one_turn_data(name):
    """Guard 4a: at most 5 % of the probes are refused; the planted uniforms are on the grid, a quarter each at
    and just below a boundary; the game after the planted turn is the first-legal one."""
    case = R.one_turn_case(name)
    assert case.n_dropped <= 0.05 * case.n_probes, (case.n_dropped, case.n_probes)
    n = len(case.u)
    assert 0.2 * n <= (case.group == 1).sum() <= 0.3 * n and 0.2 * n <= (case.group == 2).sum() <= 0.3 * n
    assert np.all(case.on <= (case.group > 0))
    # exactly ON a boundary (thr == S_i: the `<=` of the rule decides, `<` would draw the cell before): the data allow it
    # only where T / gcd(T, S_i) is a power of two -- 9, 16 and 27 of the rich sets' ~1,026 group-1 probes, hundreds of the
    # others'.  At least 5 per set, so the tie rule is never left untested
    assert (case.on & (case.group == 1)).sum() >= 5, int((case.on & (case.group == 1)).sum())
    assert np.array_equal(case.game.trace[0], case.cell.astype(np.uint8)) and case.game.kept.all()
    again = R.draw(case.own, case.opp, *R.set_by_name(name)[1:], np.where(case.on, case.u - np.float32(R.GRID), case.u))
    assert np.all(again[case.on & (case.group == 1)] < case.cell[case.on & (case.group == 1)])   # ON: one step decides


@pytest.mark.parametrize("name", sorted(R.PHILOX_KEYS))
def test_philox_games(name):
    """Guard 4b: at most 5 % of the whole games are dropped, and a kept one crosses into the second Philox draw of the
    16- and 8-lane kernels (more than 64 turns)."""
    own, opp, games = R.philox_case(name)
    assert len(own) == R.PHILOX_N and (~games.kept).sum() <= 0.05 * R.PHILOX_N
    assert (games.n_turns[games.kept] > 64).any()
    assert np.all(games.n_turns % 2 == 0)


@pytest.mark.parametrize("which", ["shipped", "random"])
def test_extreme_uniform_games_are_mostly_decided(which):
    """Guard 4c: under u = 1 - 2^-24 at most 5 % of the boards meet a boundary of the float64 CDF within 1e-5 of u."""
    games = R.extreme_case(which)[0]
    assert (~games.kept).sum() <= 0.05 * R.EXTREME_N, int((~games.kept).sum())


def test_extreme_uniform_reaches_the_fixup_branch():
    """Guard 5: the turns of the u = 1 - 2^-24 games on the shipped weights, with the float32 numerators rebuilt from
    the built table (bias, then the six (ky, plane) factors, ky-major), the lane totals ((e0 + e1) + e2) + e3 and the
    inclusive shift-1/2/4/8 scan over the 16 lanes that rollout_row_body.hpp's comments describe: where the last
    lane's own running sum (its exclusive prefix + its total) is BELOW the scanned total, u * total can reach it and
    the count is 64 -- the any_bad branch.  This restates a summation order from the kernel's comments; it is used
    ONLY to count that the branch is reached, never as an expected value."""
    from iago_amd import _lib, ops
    w, b, _ = R.real_weights("shipped")
    blob = ops.RolloutWeights(w, b, device="cpu").table.numpy()
    n_e = 3 * 2 * 2 * 256 * 4
    assert _lib.ROLLOUT_MODE_INDEX == n_e + 64
    E, bias = blob[:n_e].reshape(3, 2, 2, 256, 4), blob[n_e:n_e + 64]
    _, own, opp = R.extreme_case("shipped")
    rows = (R._rows(opp), R._rows(own))
    e = np.tile(bias[None, :], (len(own), 1)).astype(np.float32)
    for ky in range(3):
        for pl in range(2):
            fac = np.empty((len(own), 64), np.float32)
            for r in range(8):
                for half in range(2):
                    fac[:, 8 * r + 4 * half:8 * r + 4 * half + 4] = E[ky, pl, half, rows[pl][:, r + ky]]
            e = e * fac
    e = np.where(R.unpack(R.legal_moves(own, opp)).astype(bool), e, np.float32(0)).reshape(-1, 16, 4)
    assert e.dtype == np.float32
    c3 = ((e[:, :, 0] + e[:, :, 1]) + e[:, :, 2]) + e[:, :, 3]
    inc = c3.copy()
    for s in (1, 2, 4, 8):
        shifted = np.zeros_like(inc)
        shifted[:, s:] = inc[:, :-s]
        inc = inc + shifted
    below = (inc[:, 14] + c3[:, 15]) < inc[:, 15]
    assert len(below) > 10000 and below.sum() >= 100, (len(below), int(below.sum()))


def test_boundary_case():
    c = R.boundary_case()
    assert c.sure.sum() >= 0.9 * R.BOUNDARY_N, int(c.sure.sum())
    assert np.all((c.g >= 1) & (c.g <= (1 << 24) - 2))


def test_log_form_data_decide_moves_exactly():
    """The log-form case of the extremes: in the float64 oracle's own games 4,207 of 17,238 moves (u = 0) and 7,556 of
    17,290 (u = 1 - 2^-24) fall on a turn with no boundary within 1e-5 of u, where the GPU test accepts the oracle's
    draw only.  A fifth and two fifths of the moves at least, so that test is more than a legality check."""
    for u, share in ((np.float32(0), 0.2), (R.U_MAX, 0.4)):
        moves, exact = R.log_form_case(u)
        assert moves > 15000 and exact >= share * moves, (float(u), moves, exact)
