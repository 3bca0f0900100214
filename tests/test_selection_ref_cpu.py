"""The AlphaZero selection rule's restatement (tests/selection_ref.py) on hand-built trees and CPU stand-in nets, and the
library's and the engine's arguments for it: the scores of a three-child tree against numbers worked out here, what the
first selections under a fresh expansion take under either rule, that the oracle is the golden one outside the block,
that the two rules build different trees and choose different moves at the GPU tests' sizes, and what
engine.selection_arg, the engine's constructor, check_args and iago_mcts_prune_visits_rule accept and refuse."""
import ctypes as C
import math
import os
import re
import subprocess
import types

import numpy as np
import pytest

from iago_amd import _lib, engine
from oracle import mcts_py
from oracle import oracle as orc
from tests import forced_ref, negamax_ref, selection_ref, wave_mcts
from tests.gpu_util import state_of
from tests.test_oracle_golden import test_mcts_playouts as golden_mcts_playouts
from tests.test_oracle_golden import test_node_math as golden_node_math
from tests.test_wave_oracle_cpu import StandIn, _rollouts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
# The restatement is held against a library that has the rule: the engine's argument and the flag are resolved here, so
# on a tree without the feature this module does not import and every test of it fails
SELECTION_ARG, PUCT_AZ = engine.selection_arg, _lib.SEARCH_PUCT_AZ


def test_rule_is_restored():
    saved = (mcts_py.Node.__init__, mcts_py.Node.U, wave_mcts.WaveNode.select_wave, forced_ref.puct_score)
    with pytest.raises(RuntimeError):
        with selection_ref.rule():
            assert mcts_py.Node.U is selection_ref.node_u and forced_ref.puct_score is selection_ref.puct_score
            raise RuntimeError("inside")
    assert (mcts_py.Node.__init__, mcts_py.Node.U, wave_mcts.WaveNode.select_wave, forced_ref.puct_score) == saved


def _three(rule_on):
    """A root of 4 visits with children of prob 0.5 / 0.25 / 0.125, 2 / 1 / 0 visits and Q 0.25 / -0.5 / 0."""
    root = mcts_py.Node(None, 1.0)
    root.expand([(19, F32(0.5)), (26, F32(0.25)), (37, F32(0.125))])
    root.n_visits = 4
    for a, n, q in ((19, 2, 0.25), (26, 1, -0.5)):
        root.children[a].n_visits, root.children[a].Q = n, F32(q)
    return root


def test_scores_of_a_hand_built_tree():
    """c_puct = 1.5.  Under the rule P = prob and the denominator is 1 + n; outside it P = prob + 0.1 and 0.01 + n.  Every
    product and quotient is rounded on its own: float32 c_puct * P, then float64."""
    with selection_ref.rule():
        root = _three(True)
        assert float(root.P) == float(F32(F32(1.0) + F32(0.1)))          # a node without a parent keeps + 0.1
        assert [float(ch.P) for ch in root.children.values()] == [0.5, 0.25, 0.125]
        a, ch = root.select(1.5)
        got = [float(c.Q) + c.u for c in root.children.values()]
        single = mcts_py.Node(root, 1)
        assert single.P == F32(1.0) and isinstance(single.P, F32)        # the lone child: 1.0, not 1.1
    # sqrt(4) = 2; c_puct * P = 0.75, 0.375, 0.1875 exactly
    want = [0.25 + 0.75 * 2.0 / 3.0, -0.5 + 0.375 * 2.0 / 2.0, 0.0 + 0.1875 * 2.0 / 1.0]
    assert got == want and a == 19
    assert want[1] == -0.125 and want[2] == 0.375                      # (0.75: the visited favourite stays ahead)
    ref = _three(False)
    a, ch = ref.select(1.5)
    got = [float(c.Q) + c.u for c in ref.children.values()]
    ps = [F32(F32(p) + F32(0.1)) for p in (0.5, 0.25, 0.125)]
    assert [c.P for c in ref.children.values()] == ps
    want = [q + float(F32(F32(1.5) * p)) * 2.0 / (0.01 + n) for p, q, n in zip(ps, (0.25, -0.5, 0.0), (2, 1, 0))]
    assert got == want and a == 37                                       # the unvisited child's hundredfold bonus wins
    # the wave search's score and the pruning's, under the rule: the same denominator
    with selection_ref.rule():
        assert forced_ref.puct_score(1.5, F32(0.25), F32(-0.5), 1, 2.0) == -0.125
        w = wave_mcts.WaveNode(None, 1.0)
        w.expand([(19, F32(0.5)), (26, F32(0.25))])
        w.n_visits, w.vv = 3, 1
        w.children[19].n_visits, w.children[19].Q, w.children[19].vv = 2, F32(0.25), 1
        a, ch = w.select_wave(1.0, 1.0)
        # child 19: n + vv = 3, Q_eff = (0.25 * 2 - 1) / 3, u = 0.5 * 2 / (1 + 3); child 26: 0.25 * 2 / 1
        assert (0.25 * 2 - 1.0) / 3 + 0.5 * 2.0 / 4.0 < 0.5 and a == 26
    assert forced_ref.puct_score(1.5, F32(0.25), F32(-0.5), 1, 2.0) == -0.5 + float(F32(F32(1.5) * F32(0.25))) * 2.0 / 1.01


def test_first_selection_under_a_fresh_expansion():
    """Every child unvisited, Q = 0.  The new rule: the highest prior.  The reference's: the score is cp sqrt(N) / 0.01 --
    a hundred times cp sqrt(N) --, the highest stored prior too, and of children that tie there the lowest-indexed."""
    probs = [(19, F32(0.125)), (26, F32(0.5)), (37, F32(0.25)), (44, F32(0.5))]
    with selection_ref.rule():
        root = mcts_py.Node(None, 1.0)
        root.expand(probs)
        root.n_visits = 9
        a, ch = root.select(1.0)
        assert a == 26 and ch.u == 0.5 * 3.0 / 1.0
    root = mcts_py.Node(None, 1.0)
    root.expand(probs)
    root.n_visits = 9
    a, ch = root.select(1.0)
    cp = float(F32(F32(0.5) + F32(0.1)))
    assert a == 26 and ch.u == cp * 3.0 / 0.01 and root.children[44].u == ch.u
    assert ch.u == pytest.approx(100 * cp * math.sqrt(9), rel=1e-12)


def _visit_order(priors, n):
    """The children n selections take, one after the other, from a root visited once; a child's visit is worth +0.5 at the
    first child and -0.5 at the others (update_recursive up to the root, as a playout's)."""
    root = mcts_py.Node(None, 1.0)
    root.update(F32(0.0))
    root.expand([(a, F32(p)) for a, p in enumerate(priors)])
    order = []
    for _ in range(n):
        a, ch = root.select(1.0)
        order.append(a)
        ch.update_recursive(F32(0.5 if a == 0 else -0.5))
    return order


def test_second_visits():
    """The reference's rule: nobody gets a second visit before every child has one.  The new rule: a strong prior does."""
    priors = [0.7, 0.1, 0.1, 0.05, 0.05]
    ref = _visit_order(priors, 8)
    assert sorted(ref[:5]) == [0, 1, 2, 3, 4]
    with selection_ref.rule():
        az = _visit_order(priors, 8)
    assert az[:2] == [0, 0] and len(set(az[:5])) < 5


def test_outside_the_block_the_oracle_is_the_golden_one(golden_json):
    """The golden node maths and the golden trees, after a block has come and gone -- and NOT inside one."""
    with selection_ref.rule():
        with pytest.raises(AssertionError):
            golden_node_math(golden_json)
    golden_node_math(golden_json)
    golden_mcts_playouts(golden_json)


def _searches(own, opp, n_thr, nets, n_sims=100, n_sims2=37):
    """The GPU tests' two searches (100 playouts, update_with_move, 37 from the other side) on stand-in nets."""
    out = []
    for g in range(len(own)):
        m = mcts_py.MCTS(nets.policy_fn, nets.value_fn, _rollouts(100 + g), lmbda=0.5, c_puct=1.0, n_thr=n_thr)
        s = state_of(own[g], opp[g])
        a = m.get_move(s, 1, n_sims)
        first = mcts_py.dump_tree(m.root, max_depth=64)
        m.update_with_move(-1 if a is None else a)
        orc.place_stone(s, -1 if a is None else a, 1)
        m.get_move(s, 2, n_sims2)
        out.append((a, first, mcts_py.dump_tree(m.root, max_depth=64)))
    return out


@pytest.mark.parametrize("n_thr", [15, 1])
def test_the_rules_differ_at_the_gpu_tests_sizes(golden_rules, n_thr):
    """Non-vacuity of tests/test_selection_gpu.py: on the positions it checks, at its playouts and thresholds, the two
    rules build different trees and choose a different move in at least one position; together with the negamax rule
    likewise."""
    from tests.test_mcts_production_gpu import _positions
    own, opp = _positions(24, golden_rules)
    checked = [0, 1, 2, 3, 4, 12, 13, 14, 15, 16]
    own, opp = [own[g] for g in checked], [opp[g] for g in checked]
    nets = StandIn(7)
    ref = _searches(own, opp, n_thr, nets)
    with selection_ref.rule():
        az = _searches(own, opp, n_thr, nets)
        with negamax_ref.rule():
            both = _searches(own, opp, n_thr, nets)
    with negamax_ref.rule():
        neg = _searches(own, opp, n_thr, nets)
    assert sum(a[1] != r[1] for a, r in zip(az, ref)) >= 5 and sum(a[2] != r[2] for a, r in zip(az, ref)) >= 5
    assert any(a[0] != r[0] for a, r in zip(az, ref))
    assert any(b[2] != a[2] for b, a in zip(both, az)) and any(b[2] != n[2] for b, n in zip(both, neg))
    # the dead and the full board: a chain of pass children, 1.0 under the rule and 1.1 under the reference's
    for g in (2, 3):
        assert az[g][0] == ref[g][0] == -1 and az[g][1]["order"] == ref[g][1]["order"] == [-1]
        assert az[g][1]["children"]["-1"]["P"] == 1.0 and ref[g][1]["children"]["-1"]["P"] == float(F32(F32(1.0) + F32(0.1)))


def test_selection_arg():
    assert SELECTION_ARG("reference") == "reference" and SELECTION_ARG("alphazero") == "alphazero"
    for bad in (None, "", "AlphaZero", b"alphazero", 0, 1, True, ("alphazero",)):
        with pytest.raises(ValueError):
            SELECTION_ARG(bad)


@pytest.mark.parametrize("kw", [dict(selection="puct"), dict(selection=None), dict(selection="alphazero", persistent=False),
                                dict(selection="alphazero", use_graph=True), dict(selection="alphazero", async_steps=True),
                                dict(selection="alphazero", lookahead=4)])
def test_engine_refuses_before_it_allocates(kw):
    """A bad string, or "alphazero" with the per-playout launches asked for: ValueError before anything is allocated (no
    device is touched: this runs without one)."""
    from iago_amd import engine
    with pytest.raises(ValueError, match="selection"):
        engine.BatchedMCTS(1, None, None, None, **kw)


def test_a_rollout_hook_on_an_alphazero_engine_is_refused():
    """The check that guards negamax guards this rule: an engine's shell is enough to see it."""
    from iago_amd import engine
    m = engine.BatchedMCTS.__new__(engine.BatchedMCTS)
    m.backup, m.selection, m.persistent, m.rollout_hook = "reference", "alphazero", True, (lambda e: None)
    with pytest.raises(ValueError, match="alphazero"):
        m._backup_check()
    with pytest.raises(ValueError, match="alphazero"):
        m.search(None, None, None, 10)
    with pytest.raises(ValueError, match="alphazero"):
        engine.SelfPlayEngine._play(types.SimpleNamespace(mcts=m), 10, None, True, engine.NO_RULES)
    m.rollout_hook = None
    m._backup_check()
    m.selection, m.rollout_hook = "reference", (lambda e: None)
    m._backup_check()


def test_flag_and_bindings():
    text = open(os.path.join(ROOT, "include", "iago_hip_serving.h")).read()
    assert int(re.search(r"#define IAGO_SEARCH_PUCT_AZ (0x[0-9a-fA-F]+)", text).group(1), 16) == PUCT_AZ == 0x400
    assert _lib.SEARCH_PUCT_AZ & (_lib.SEARCH_NEGAMAX | _lib.SEARCH_CHAIN_SKIP) == 0
    assert _lib.SEARCH_GAMES_PER_WORKGROUP < min(_lib.SEARCH_PUCT_AZ, _lib.SEARCH_NEGAMAX, _lib.SEARCH_CHAIN_SKIP)
    assert "IAGO_SEARCH_PUCT_AZ" not in open(os.path.join(ROOT, "include", "iago_hip.h")).read()


@pytest.mark.parametrize("gpw,refused", [(7 | 0x400, True), (7 | 0x700, True), (8 | 0x400, False), (32 | 0x700, False),
                                         (0x400, False)])
def test_library_strips_all_three_flags(gpw, refused):
    """check_args reads games_per_workgroup without its three flags: 7 is refused by name whatever flags it carries, 8 / 32
    / 0 (= 32) pass that check (and are refused later: these argument sets cannot be launched)."""
    from tests.test_search_refusals_cpu import Call
    c = Call("persistent")
    c.a.games_per_workgroup = gpw
    rc, msg = c()
    assert rc != 0
    assert (b"games_per_workgroup is 0 (= 32), 8, 16 or 32" in msg) == refused, msg


def test_prune_visits_rule_is_declared_exported_and_refuses():
    from iago_amd import _lib as L, build
    from tests.test_forced_ref_cpu import K256, _refused
    from tests.test_search_refusals_cpu import Call
    so = build.build()
    text = open(os.path.join(ROOT, "include", "iago_hip_serving.h")).read()
    declared = set(re.findall(r"IAGO_API[^;(]*?\b(iago_\w+)\s*\(", text))
    name = "iago_mcts_prune_visits_rule"
    assert name in declared and name in L.SERVING_SYMBOLS and hasattr(L.lib(), name)
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    assert name in set(re.findall(r" T (iago_\w+)", out))
    assert name not in open(os.path.join(ROOT, "include", "iago_hip.h")).read()
    lib = L.lib()
    one = Call("persistent")
    f = 0x7E0000200000
    who = name.encode()

    def call(tree, k, flags, out):
        return lib.iago_mcts_prune_visits_rule(tree, None, 1.0, k, flags, out, None), lib.iago_last_error()
    for flags in (1, 0x100, 0x200, 0x401, 0x800, -1):
        _refused(call(C.byref(one.tree), K256, flags, f), who, b"flags")
    for flags in (0, L.SEARCH_PUCT_AZ):     # what iago_mcts_prune_visits refuses, under either rule
        _refused(call(None, K256, flags, f), who, b"bad tree")
        for k in (0, -1, 4097):
            _refused(call(C.byref(one.tree), k, flags, f), who, b"k_256")
        _refused(call(C.byref(one.tree), K256, flags, None), who, b"null pruned")
    # the sibling keeps its name in its refusals
    rc = lib.iago_mcts_prune_visits(C.byref(one.tree), None, 1.0, 0, f, None)
    assert rc != 0 and lib.iago_last_error().startswith(b"iago_mcts_prune_visits: k_256")
