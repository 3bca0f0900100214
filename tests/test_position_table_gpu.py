"""The position table of the persistent search (tests/table_util.py: its layout and its reader's rule) where two agents
meet on one entry.  At its default 2^20 slots a put and a get almost never touch the same entry within the same
microseconds, so every other test sees the table after the fact.  IAGO_PERSISTENT_TABLE shrinks it -- to ONE slot, where
every lookup and every put of every game is a collision or an eviction.

  a. planted entries: one search of one game from the start position on a one-slot table whose entry the test wrote
     before the launch.  The first lookup of the launch is the fresh root's.  A valid entry of the root is taken (the
     positive control: the reader does consult the slot); an entry that breaks exactly ONE clause of the reader's rule
     -- sequence word 0, sequence word odd, the value word's sequence number another one, opp one stone more, own one
     stone more, own and opp swapped -- is not, and the search is the search without a table, bit for bit; the sequence
     number wraps from 0xFFFFFFFE to 2, not to 0.
  b. contention: 64 games that start from one position ask for the same positions at the same moments.  The trees, the
     stored values, the rollout results and the number of fresh leaves are those of the search without a table, for a
     table of 1, 2, 64 and 4096 slots; so are the role split's, the wave search's, whole games' in one launch and a
     search whose idle net workgroups walk values ahead, on 1 and 64 slots.  What is left in the table afterwards passes
     table_util.audit.
  c. a size that is no power of two is refused by the library.

Hit counts (totals[8]) depend on timing: HITS_MEASURED holds the smallest count of three runs of block b per (case,
slots) (LABNOTES.md, "The position table under contention and with planted entries").  Where it is at least 20 a run
must have hits -- without any it proves nothing about accepted reads.  Below 20, nothing is asserted about the hits:
role-split, wave-32 and values-ahead on 1 slot, whole-games on 1 and on 64 slots."""
import numpy as np
import pytest
import torch

from tests import table_util as tu
from tests.test_negamax_gpu import RECORDS, _same
from tests.test_search_persistent_gpu import _positions, nets  # noqa: F401  (the fixture: random-initialised nets)
from tests.test_search_wave_gpu import _engine as _wave_engine, _two_searches

pytestmark = pytest.mark.gpu

START_OWN, START_OPP = 0x0000000810000000, 0x0000001008000000
TREE = ("n_visits", "q", "p", "first_child", "parent", "action", "n_children", "n_nodes", "root")
LOGS = ("z_log", "z_log_n", "leaf_value")

# (case, slots): the smallest totals[8] of three runs of block b (LABNOTES.md).  At least 20: a run must count hits.
# Below 20, nothing asserted about the hits: one slot under 16 or 48 games or two wave trees (5 to 15 hits), and whole
# games at either size -- the 8 games are one workgroup's, they reach a shared position in the same iteration, before
# anybody's put, and part ways within a few moves (0 or 1 hit in 2530 fresh leaves)
HITS_MEASURED = {
    ("games-64", 1): 37, ("games-64", 2): 39, ("games-64", 64): 462, ("games-64", 4096): 770,
    ("role-split", 1): 5, ("role-split", 64): 91, ("wave-32", 1): 10, ("wave-32", 64): 22,
    ("whole-games", 1): 0, ("whole-games", 64): 0, ("values-ahead", 1): 5, ("values-ahead", 64): 393,
}
HITS_ASSERTED = {k for k, n in HITS_MEASURED.items() if n >= 20}
HITS_NOT_ASSERTED = set(HITS_MEASURED) - HITS_ASSERTED


def _search(nets, G, n_sims, n_sims2, own, opp, before=None, **kw):
    """tests/test_search_persistent_gpu.py's _run with a hook between the engine's construction and its first search.
    Returns (engine, host copies of what it built, the root's own / opp of the first search)."""
    engine, ops, policy, value, rw = nets
    m = engine.BatchedMCTS(G, policy, value, rw, n_thr=15, capacity=engine.suggest_capacity(n_sims + n_sims2, 15, moves=2),
                           seed=21, game_id_base=300, z_log_rows=n_sims + n_sims2, persistent=True, **kw)
    if before is not None:
        before(m)
    o, p = ops.bits_to_tensor(own), ops.bits_to_tensor(opp)
    active = torch.ones(G, dtype=torch.uint8, device="cuda")
    m.search(o, p, active, n_sims)
    if n_sims2:
        mv = m.best_move(active)[0].clone()
        mv = torch.where(mv == -2, torch.full_like(mv, -1), mv)
        m.update_with_move(mv, active.clone())
        ops.apply_moves(o, p, mv)
        m.search(p, o, active, n_sims2)
    torch.cuda.synchronize()
    t = m.tree
    out = {k: getattr(t, k).cpu().numpy().copy() for k in TREE + ("v",)}
    out["first_child"] = np.where(out["first_child"] < 0, -1, out["first_child"])
    out["z_log"], out["z_log_n"] = m.z_log.cpu().numpy().copy(), m.z_log_n.cpu().numpy().copy()
    out["leaf_value"] = m.leaf_value.cpu().numpy().copy()
    # no launch gave up, no pool overflowed (search() raises on either; the words themselves, too)
    assert int(m._ps["ctl"][3].item()) == 0 and int(t.overflow.sum().item()) == 0
    return m, out


def _differing(a, b):
    """The comparison keys in which two runs differ: the trees, the NaN pattern of v and its other values as bits, the
    rollout results and the leaf values."""
    bad = [k for k in TREE + LOGS if not np.array_equal(a[k], b[k])]
    na, nb = np.isnan(a["v"]), np.isnan(b["v"])
    if not np.array_equal(na, nb):
        bad.append("v: NaN pattern")
    elif not np.array_equal(a["v"][~na].view(np.uint32), b["v"][~nb].view(np.uint32)):
        bad.append("v")
    return bad


def _counts(m):
    """(fresh leaves asked for, table hits, hits on the asking game's own entries, values walked ahead)."""
    tot = m._ps["totals"].cpu().numpy()
    return m.n_value_inline, int(tot[8]), int(tot[12]), m.n_value_ahead


def _root_bits(out, g=0):
    cap = out["v"].shape[0] // out["root"].shape[0]
    return int(out["v"].view(np.uint32)[g * cap + out["root"][g]])


def _with_env(env):
    mp = pytest.MonkeyPatch()
    for k, v in env.items():
        mp.setenv(k, v)
    return mp


# ---------------------------------------------------------------------------------------------------- a. planted entries

ONE = (np.array([START_OWN], np.uint64), np.array([START_OPP], np.uint64))
A_SIMS = 40


@pytest.fixture(scope="module")
def no_table(nets):
    """T0, V0, N0: the search of block a without a table."""
    mp = _with_env({"IAGO_PERSISTENT_TABLE": "0"})
    try:
        m, out = _search(nets, 1, A_SIMS, 0, *ONE, lmbda=0.5)
        assert m._vtable is None
        n0 = m.n_value_inline
        m.close()
    finally:
        mp.undo()
    v0 = _root_bits(out)
    assert v0 != 0x7FC00000 and n0 > 1 and not np.isnan(out["v"][out["root"][0]])
    return out, v0, n0


def _planted_value(v0):
    """The bits of a float that is not V0."""
    bits = tu.float_bits(0.625)
    return bits if bits != v0 else tu.float_bits(-0.625)


def _planted_search(nets, monkeypatch, words):
    monkeypatch.setenv("IAGO_PERSISTENT_TABLE", "1")

    def before(m):
        assert m._vtable is not None and m._vtable.numel() == 4
        tu.plant(m, 0, *words)
        assert tu.read(m)[0].tolist() == [w & 0xFFFFFFFFFFFFFFFF for w in words]

    return _search(nets, 1, A_SIMS, 0, *ONE, before=before, lmbda=0.5)


def test_a_planted_valid_entry_is_taken(nets, no_table, monkeypatch):
    """The positive control: a published entry of the root's position is what the root's first visit takes."""
    t0, v0, n0 = no_table
    bits = _planted_value(v0)
    m, out = _planted_search(nets, monkeypatch, (tu.seq_word(2), START_OWN, START_OPP, tu.value_word(2, bits)))
    inline, hits, own_hits, _ = _counts(m)
    m.close()
    print("planted valid entry: root bits %#x (planted %#x, V0 %#x), hits %d, asked %d, N0 %d" % (
        _root_bits(out), bits, v0, hits, inline, n0))
    assert _root_bits(out) == bits
    assert hits >= 1
    assert inline + hits == n0
    assert _differing(out, t0) != []


B0, B63 = 1 << 0, 1 << 63          # two corners: empty at the root, and a position of those two stones alone is no game's
REJECTED = {
    # row: (sequence number, the value word's sequence number, own, opp)
    "sequence-word-zero": (0, 0, START_OWN, START_OPP),
    "sequence-word-odd": (3, 3, START_OWN, START_OPP),
    "value-word-of-another-sequence": (2, 4, START_OWN, START_OPP),
    "opp-one-stone-more": (2, 2, START_OWN, START_OPP | B0),
    "own-one-stone-more": (2, 2, START_OWN | B0, START_OPP),
    "own-and-opp-swapped": (2, 2, START_OPP, START_OWN),
    "sequence-wraps": (0xFFFFFFFE, 0xFFFFFFFE, B0, B63),
}


@pytest.mark.parametrize("row", list(REJECTED))
def test_a_planted_entry_that_breaks_one_clause_is_not_taken(nets, no_table, monkeypatch, row):
    """Each row is a published-looking entry that carries the bits of a float that is not V0 and differs from a valid
    entry of the root in ONE respect, the one its clause of vtable_get tests (the rows with sequence word 0 and 3 carry
    that number in their value word, too: nothing else rejects them).  The search must be the search without a table.
    sequence-word-odd: no writer touches the slot either (vtable_put_begin leaves a slot that is being written alone),
    so there is no hit at all and the four words stay.  value-word-of-another-sequence: a later put replaces the entry
    with a consistent one.  sequence-wraps: a valid entry of a position no search reaches, one put below the wrap; the
    number after it is 2, never 0 (0 = never used) and never odd."""
    t0, v0, n0 = no_table
    s, vs, own, opp = REJECTED[row]
    words = (tu.seq_word(s), own, opp, tu.value_word(vs, _planted_value(v0)))
    m, out = _planted_search(nets, monkeypatch, words)
    inline, hits, own_hits, _ = _counts(m)
    after = tu.read(m)[0]
    print("%s: differing %r, root bits %#x (V0 %#x), hits %d, asked %d (N0 %d), slot 0 afterwards %s" % (
        row, _differing(out, t0), _root_bits(out), v0, hits, inline, n0, [hex(int(w)) for w in after]))
    try:
        assert _differing(out, t0) == []
        assert _root_bits(out) == v0
        if row == "sequence-word-odd":
            assert hits == 0
            assert after.tolist() == [w & 0xFFFFFFFFFFFFFFFF for w in words]
        else:
            assert inline + hits == n0
        if row in ("value-word-of-another-sequence", "sequence-wraps"):
            assert tu.audit(m, nets[3])[0] == 1
        if row == "sequence-wraps":
            seq = int(after[0]) & 0xFFFFFFFF
            assert seq != 0 and seq % 2 == 0 and seq < 1 << 31
    finally:
        m.close()


# -------------------------------------------------------------------------------------------------------- b. contention

def _start(G):
    return np.full(G, START_OWN, np.uint64), np.full(G, START_OPP, np.uint64)


def _run_main(nets):
    return _search(nets, 64, 100, 45, *_start(64))


def _run_split(nets):
    m, out = _search(nets, 16, 100, 45, *_start(16), split=8)
    assert m._split is not None and m.split_cus == 8      # the net workgroups: another launch on another stream
    return m, out


def _run_ahead(nets):
    return _search(nets, 48, 100, 45, *_positions(48))


def _run_wave(nets):
    m = _wave_engine(nets, 2, 64, wave=32)
    active = torch.ones(2, dtype=torch.uint8, device="cuda")
    first, second, _ = _two_searches(m, *_start(2), active, 64)
    assert int(m._ps["ctl"][3].item()) == 0 and int(m.tree.overflow.sum().item()) == 0
    return m, (first, second)


def _run_games(nets):
    engine, ops, policy, value, rw = nets
    m = engine.BatchedMCTS(8, policy, value, rw, n_thr=15, capacity=4096, seed=11, game_id_base=70, persistent=True)
    r = engine.SelfPlayEngine(m).play(20)
    assert r.launches == 1 and r.game_turns is not None    # whole games, every turn of them, in ONE launch
    assert int(m._ps["ctl"][3].item()) == 0 and int(m.tree.overflow.sum().item()) == 0
    out = {k: getattr(r, k).cpu().numpy().copy() for k in RECORDS}
    out["n_turns"] = r.n_turns
    return m, out


def _same_searches(a, b):
    assert _differing(a, b) == []


def _same_waves(a, b):
    for x, y in zip(a, b):
        assert torch.equal(x["nodes"], y["nodes"]) and torch.equal(x["n_nodes"], y["n_nodes"])
        assert np.array_equal(x["zlog"], y["zlog"])


# case: (the run, the comparison, IAGO_PERSISTENT_AHEAD)
CASES = {
    "games-64": (_run_main, _same_searches, "-1"),
    "role-split": (_run_split, _same_searches, "-1"),
    "wave-32": (_run_wave, _same_waves, "-1"),            # (a wave's slots: compared as the wave tests compare them)
    "whole-games": (_run_games, _same, "-1"),
    "values-ahead": (_run_ahead, _same_searches, "1"),
}
_BASE = {}


def _baseline(case, nets):
    """The case's run without a table, once per module."""
    if case not in _BASE:
        run, _, ahead = CASES[case]
        mp = _with_env({"IAGO_PERSISTENT_TABLE": "0", "IAGO_PERSISTENT_AHEAD": ahead})
        try:
            m, out = run(nets)
            assert m._vtable is None and _counts(m)[1:] == (0, 0, 0)
            _BASE[case] = (out, m.n_value_inline)
            m.close()
        finally:
            mp.undo()
    return _BASE[case]


def _contend(case, slots, nets, monkeypatch):
    run, same, ahead = CASES[case]
    want, n0 = _baseline(case, nets)
    monkeypatch.setenv("IAGO_PERSISTENT_TABLE", str(slots))
    monkeypatch.setenv("IAGO_PERSISTENT_AHEAD", ahead)
    m, got = run(nets)
    try:
        assert (m._vtable is None) == (slots == 0) and (slots == 0 or m._vtable.numel() == 4 * slots)
        inline, hits, own_hits, n_ahead = _counts(m)
        left = tu.audit(m, nets[3])[0] if slots else 0
        print("contention %s, %d slots: totals[8] %d, totals[12] %d, n_value_ahead %d, asked %d (no table: %d), entries "
              "left %d" % (case, slots, hits, own_hits, n_ahead, inline, n0, left))
        same(got, want)
        assert inline + hits == n0              # the same fresh leaves either way: asked for, or found in the table
        assert own_hits <= hits
        assert 0 < left <= slots or slots == 0
        if (case, slots) in HITS_ASSERTED:
            assert hits > 0
        return n_ahead
    finally:
        m.close()


@pytest.mark.parametrize("slots", [0, 1, 2, 64, 4096])
def test_b_trees_do_not_depend_on_the_tables_size(nets, monkeypatch, slots):
    """64 games from the start position, distinct game ids, 100 playouts, a move, 45 playouts; no values ahead."""
    _contend("games-64", slots, nets, monkeypatch)


@pytest.mark.parametrize("slots", [1, 64])
@pytest.mark.parametrize("case", ["role-split", "wave-32", "whole-games", "values-ahead"])
def test_b_other_launch_forms_on_a_small_table(nets, monkeypatch, case, slots):
    """role-split: split=8, 16 games.  wave-32: two trees, 64 + 60 playouts.  whole-games: 8 games of 20 playouts per
    move through SelfPlayEngine.play.  values-ahead: 48 games with IAGO_PERSISTENT_AHEAD=1 -- idle net workgroups put
    entries nobody waits for."""
    n_ahead = _contend(case, slots, nets, monkeypatch)
    if case == "values-ahead" and slots == 64:
        assert n_ahead > 0


# ----------------------------------------------------------------------------------------------- c. the knob's other values

def test_c_a_size_that_is_no_power_of_two_is_refused(nets, monkeypatch):
    from iago_amd import _lib
    engine, ops, policy, value, rw = nets
    monkeypatch.setenv("IAGO_PERSISTENT_TABLE", "1000")
    m = engine.BatchedMCTS(1, policy, value, rw, n_thr=15, capacity=256, seed=21, persistent=True)
    assert m._vtable.numel() == 4000
    with pytest.raises(_lib.IagoError, match="vtable_slots"):
        m.search(ops.bits_to_tensor(ONE[0]), ops.bits_to_tensor(ONE[1]), torch.ones(1, dtype=torch.uint8, device="cuda"), 4)
    m.close()
