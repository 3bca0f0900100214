"""The remembered pass chain of the persistent search's descent (csrc/search_kernel.hip, descend; BatchedMCTS(chain_skip=),
IAGO_SEARCH_CHAIN_SKIP): a game that stands where its last playout's path turned into a run of pass levels -- nodes with
ONE child, a pass (MCTS.py:109-117) -- takes the rest of that path from the path buffer instead of walking it.  Timing
only: trees, stored values, visit rows, moves, records, z, final boards and overflow flags are those of the walk
(chain_skip=False) byte for byte, in every launch form that shares the game workgroup and on both homes of the path buffer
(a workgroup's LDS; the caller's array, which a path_stride too large for the LDS selects), and the single searches are
those of the per-playout engine (descend_kernel, which has no such shortcut) node for node.  totals[16] counts the levels
jumped over: > 0 wherever the switch is on, 0 where it is off."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests.conftest import load_json

pytestmark = pytest.mark.gpu

RECORDS = ("own", "opp", "valid", "move", "pi", "z", "final_p1", "final_p2")
TREE = ("n_visits", "q", "p", "first_child", "parent", "action", "n_children", "n_nodes", "root", "v", "overflow")
GLOBAL_STRIDE = 8192   # (8 paths of 8192 entries: 256 KB, more than a CU's LDS -> the paths live in the caller's array)


@pytest.fixture(scope="module")
def nets():
    from iago_amd import engine, network, ops
    assert torch.cuda.is_available()
    torch.manual_seed(3)
    policy = network.SLPolicy().cuda().eval()          # random init: broad trees
    value = network.Value().cuda().eval()
    g = load_json("simulate.json")
    return engine, ops, policy, value, ops.RolloutWeights(g["shipped_w"], g["shipped_b"])


def _trees(m):
    t = m.tree
    out = {k: getattr(t, k).cpu().numpy().copy() for k in TREE}
    out["first_child"] = np.where(out["first_child"] < 0, -1, out["first_child"])   # (a leaf either way)
    return out


def _same(a, b, keys):
    for k in keys:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k   # (byte-equal: NaN = NaN)


def _games(nets, G, n_sims, n_thr, how="play", **kw):
    """G whole self-play games in one launch (how: "play", ("stream", n_games) or ("solve", k))."""
    engine, ops, policy, value, rw = nets
    m = engine.BatchedMCTS(G, policy, value, rw, n_thr=n_thr, seed=11, game_id_base=300, persistent=True,
                           capacity=engine.suggest_capacity(n_sims, n_thr, moves=64), **kw)
    if kw.get("split"):
        assert m._split is not None and m.split_cus == kw["split"]
    e = engine.SelfPlayEngine(m)
    if how == "play":
        r = e.play(n_sims)
    elif how[0] == "stream":
        r = e.play_stream(n_sims, how[1])
    else:
        r = e.play(n_sims, solve_empties=how[1])
    out = {k: getattr(r, k).cpu().numpy() for k in RECORDS}
    out["game_turns"] = r.game_turns.cpu().numpy() if r.game_turns is not None else None
    out.update(_trees(m))
    assert r.launches == (1 if how == "play" or how[0] == "stream" else 2) and getattr(e, "n_replayed", 0) == 0
    assert int(out["overflow"].sum()) == 0
    out["skipped"] = int(m._ps["totals"][16].item())
    m.close()
    return out


WHOLE = {"100_playouts": (32, 100, 15), "n_thr_1": (8, 100, 1), "400_playouts": (8, 400, 15)}
_walked = {}


def _walk(nets, case):
    """The case with every level walked, paths in LDS: the one reference of the case's comparisons."""
    if case not in _walked:
        _walked[case] = _games(nets, *WHOLE[case], chain_skip=False)
        assert _walked[case]["skipped"] == 0
    return _walked[case]


@pytest.mark.parametrize("form", ["on_lds", "on_global", "off_global"])
@pytest.mark.parametrize("case", sorted(WHOLE))
def test_whole_games_on_equals_off_on_both_homes(nets, case, form):
    """32 games x 100 playouts, 8 games x 100 playouts at n_thr = 1 (a chain grows at every visit, paths run into the
    hundreds), 8 games x 400 playouts: the switch on and off, the paths in LDS and in the caller's array."""
    ref = _walk(nets, case)
    on = form.startswith("on")
    got = _games(nets, *WHOLE[case], chain_skip=on, path_stride=GLOBAL_STRIDE if form.endswith("global") else None)
    _same(got, ref, RECORDS + ("game_turns",) + TREE)
    assert (got["skipped"] > 0) if on else (got["skipped"] == 0)
    print(case, form, "levels jumped over:", got["skipped"])


@pytest.mark.parametrize("name,G,how,kw", [("role_split", 96, "play", dict(split=8)),
                                          ("stream", 16, ("stream", 48), {}),
                                          ("solve_empties", 32, ("solve", 2), {})])
def test_other_launch_forms_on_equals_off(nets, name, G, how, kw):
    """The role split (96 games on 8 game CUs), a stream (three times the slot count) and games that the exact solver
    plays out from 2 empties on (the search kernel's park instantiation): 100 playouts, n_thr 15."""
    on, off = (_games(nets, G, 100, 15, how, chain_skip=s, **kw) for s in (True, False))
    # (a stream: which slot plays which game is the order in which the workgroups claim ids -- timing; the records are by game)
    _same(on, off, RECORDS + ("game_turns",) + (("overflow",) if name == "stream" else TREE))
    assert on["skipped"] > 0 and off["skipped"] == 0


def _late_roots():
    """Positions of uniform-random games with 0 .. 3 empties, by (empties, kind): kind "move" (the side to move has a
    move), "pass" (it must pass and the other side then moves), "over" (neither side has a move); own = the side to move."""
    found = {}
    for game in range(400):
        _, _, tr = orc.random_playout(orc.initial_state(), 1, seed=5, game_id=game)
        s, color = orc.initial_state(), 1
        for a in list(tr) + [None]:
            empties = int((s == 0).sum())
            if empties <= 3:
                mine, theirs = len(orc.legal_actions(s, color)), len(orc.legal_actions(s, 3 - color))
                kind = "move" if mine else ("pass" if theirs else "over")
                p1, p2 = orc.state_to_bits(s)
                found.setdefault((empties, kind), (p1, p2) if color == 1 else (p2, p1))
            if a is None:
                break
            orc.place_stone(s, a, color)
            color = 3 - color
    return found


@pytest.fixture(scope="module")
def late_roots():
    found = _late_roots()
    need = [(0, "over"), (1, "move"), (2, "move"), (3, "move")]
    assert all(k in found for k in need), sorted(found)
    assert any(k[1] == "pass" for k in found) and any(k[1] == "over" and k[0] > 0 for k in found), sorted(found)
    return found


def _roots(found, G, kinds=None):
    keys = [k for k in sorted(found) if kinds is None or k[1] in kinds]
    own = np.array([found[keys[i % len(keys)]][0] for i in range(G)], np.uint64)
    opp = np.array([found[keys[i % len(keys)]][1] for i in range(G)], np.uint64)
    return own, opp


def _searches(nets, own, opp, n_sims, n_sims2, active=None, check=True, **kw):
    """Two consecutive single searches (the turn loop's form) with the most visited move (or a pass) in between."""
    engine, ops, policy, value, rw = nets
    G, n_thr = len(own), kw.pop("n_thr", 3)
    m = engine.BatchedMCTS(G, policy, value, rw, n_thr=n_thr, seed=21, game_id_base=300,
                           capacity=engine.suggest_capacity(n_sims + n_sims2, n_thr, moves=2), **kw)
    o, p = ops.bits_to_tensor(own), ops.bits_to_tensor(opp)
    act = torch.ones(G, dtype=torch.uint8, device="cuda")
    for g in (active or ()):
        act[g] = 0
    m.search(o, p, act, n_sims, check=check)
    if n_sims2:
        mv = m.best_move(act)[0].clone()
        mv = torch.where(mv == -2, torch.full_like(mv, -1), mv)
        m.update_with_move(mv, act.clone())
        ops.apply_moves(o, p, mv)
        m.search(p, o, act, n_sims2, check=check)
    out = _trees(m)
    out["leaf_value"] = m.leaf_value.cpu().numpy().copy()
    out["skipped"] = int(m._ps["totals"][16].item()) if m.persistent else 0
    m.close()
    return out


def test_single_searches_from_late_roots_equal_the_per_playout_engine(nets, late_roots):
    """Roots with 0 .. 3 empties -- the side to move has a move, must pass, or the game is over --, n_thr = 3, two searches
    per game with a move in between (a chain remembered from before update_with_move would show): node for node the trees
    of descend_kernel."""
    own, opp = _roots(late_roots, 24)
    on = _searches(nets, own, opp, 90, 60, persistent=True)
    ref = _searches(nets, own, opp, 90, 60, persistent=False, use_graph=True)
    assert int(on["overflow"].sum()) == 0 and on["skipped"] > 0
    _same(on, ref, [k for k in TREE if k != "v"] + ["leaf_value"])
    assert np.array_equal(np.isnan(on["v"]), np.isnan(ref["v"]))
    assert np.array_equal(on["v"][~np.isnan(on["v"])], ref["v"][~np.isnan(ref["v"])])


@pytest.mark.parametrize("stride,n_sims", [(8, 100), (None, 560)])
def test_overflow_reports_are_the_walk_s(nets, late_roots, stride, n_sims):
    """n_thr = 1 at roots where the game is over or nearly: the chain grows by a level per playout.  The smallest path
    buffer the engine accepts (8 entries) overflows within a dozen playouts: the same games are reported, and the trees --
    void as they are -- are the walk's.  The default one (520) leaves the descent's own bound of 512 levels to be hit first,
    which the levels jumped over count against: the walk stops at a node 512 levels down that is never backed up, so never
    expands and raises no flag -- the chain stops growing, with the switch on as with it off."""
    own, opp = _roots(late_roots, 8, kinds=("over", "pass") if stride is None else None)
    on, off = (_searches(nets, own, opp, n_sims, 0, check=False, n_thr=1, persistent=True, chain_skip=s, path_stride=stride)
               for s in (True, False))
    if stride is not None:
        assert int(off["overflow"].sum()) >= 1
    else:   # (game 0: the root with 0 empties -- the root and a chain that ran into the bound before the search ended)
        assert 500 < int(off["n_nodes"][0]) < n_sims - 30
    _same(on, off, list(TREE) + ["leaf_value"])
    assert on["skipped"] > 0 and off["skipped"] == 0


def test_a_wave_of_games_at_different_stages(nets, late_roots):
    """ONE workgroup, its eight games one wave of 64 lanes: three late roots (chains to remember), three mid-game
    positions, a root where the game is over, a game that takes no part.  The jump of one game and the walk of another
    share every loop iteration: equal to the walk and to the per-playout engine."""
    from tests.gpu_util import random_positions
    own, opp = _roots(late_roots, 8, kinds=("move", "pass"))
    mid_own, mid_opp = random_positions(3, seed=78)
    own[3:6], opp[3:6] = mid_own, mid_opp
    own[6], opp[6] = late_roots[(0, "over")]
    on, off = (_searches(nets, own, opp, 120, 50, active=(7,), persistent=True, chain_skip=s) for s in (True, False))
    ref = _searches(nets, own, opp, 120, 50, active=(7,), persistent=False, use_graph=True)
    assert int(on["overflow"].sum()) == 0 and on["skipped"] > 0 and off["skipped"] == 0
    _same(on, off, list(TREE) + ["leaf_value"])
    _same(on, ref, [k for k in TREE if k != "v"] + ["leaf_value"])
    assert on["n_nodes"][7] == 1
