"""The negamax backup rule's restatement (tests/negamax_ref.py) on CPU stand-in nets, and the engine's argument for it:
the signs along a path, the tree both rules build when every leaf is worth 0, subtree reuse against a from-scratch
recomputation by ABSOLUTE depth (the invariant does not depend on where the root is), and what engine.backup_arg and
the engine's constructor refuse."""
import types

import numpy as np
import pytest

from oracle import mcts_py
from oracle import oracle as orc
from tests import negamax_ref
from tests.test_oracle_golden import _cmp_tree
from tests.test_wave_oracle_cpu import StandIn, _rollouts


def test_rule_is_restored():
    reference = mcts_py.Node.update_recursive
    with pytest.raises(RuntimeError):
        with negamax_ref.rule():
            assert mcts_py.Node.update_recursive is negamax_ref.update_recursive
            raise RuntimeError("inside")
    assert mcts_py.Node.update_recursive is reference


def test_signs_along_a_path():
    """A hand-built path of four nodes: -, +, -, + from the leaf up; a second playout that ends one level higher turns
    every sign the nodes it shares see (the parity is the distance to THAT playout's leaf)."""
    root = mcts_py.Node(None, 1.0)
    a = mcts_py.Node(root, 0.5)
    b = mcts_py.Node(a, 0.5)     # (a pass child is a level like any other: nothing in the rule looks at the action)
    leaf = mcts_py.Node(b, 0.5)
    lv = np.float32(0.625)
    with negamax_ref.rule():
        leaf.update_recursive(lv)
    assert [n.Q for n in (leaf, b, a, root)] == [-lv, lv, -lv, lv]
    assert [n.n_visits for n in (leaf, b, a, root)] == [1, 1, 1, 1]
    assert all(isinstance(n.Q, np.float32) for n in (leaf, b, a, root))
    lv2 = np.float32(-0.25)
    with negamax_ref.rule():
        b.update_recursive(lv2)
    # Node.update's arithmetic, unchanged: Q += (v - Q) / n with v = -lv2, +lv2, -lv2 from b up
    want = [(b, lv, -lv2), (a, -lv, lv2), (root, lv, -lv2)]
    for node, q1, v in want:
        assert node.n_visits == 2 and node.Q == q1 + (v - q1) / 2
    assert leaf.n_visits == 1 and leaf.Q == -lv
    # the reference's rule on the same path: the same value at every level
    r = mcts_py.Node(None, 1.0)
    c = mcts_py.Node(r, 0.5)
    c.update_recursive(lv)
    assert (c.Q, r.Q) == (lv, lv)


@pytest.mark.parametrize("n_thr", [1, 3])
def test_zero_leaf_values_build_the_same_tree(n_thr):
    """lv == 0 at every leaf: -0 steers nothing, so both rules build the same tree (visits, P, order; Q == 0 either way)."""
    nets = StandIn(7)
    zero = lambda x: np.float32(0.0)      # noqa: E731

    def run():
        m = mcts_py.MCTS(nets.policy_fn, zero, lambda s, c: 0, lmbda=0.5, c_puct=1.0, n_thr=n_thr)
        move = m.get_move(orc.initial_state(), 1, 80)
        return move, mcts_py.dump_tree(m.root, max_depth=64)

    ref_move, ref_tree = run()
    with negamax_ref.rule():
        neg_move, neg_tree = run()
    assert ref_move == neg_move
    _cmp_tree(neg_tree, ref_tree, "lv=0")     # (-0.0 == 0.0)


def test_rules_differ_with_real_leaf_values():
    nets = StandIn(7)

    def run():
        m = mcts_py.MCTS(nets.policy_fn, nets.value_fn, _rollouts(3), lmbda=0.5, c_puct=1.0, n_thr=3)
        m.get_move(orc.initial_state(), 1, 80)
        return mcts_py.dump_tree(m.root, max_depth=64)

    ref = run()
    with negamax_ref.rule():
        neg = run()
    assert ref != neg


def _walk(node, depth, out):
    out.append((node, depth))
    for ch in node.children.values():
        _walk(ch, depth + 1, out)


def test_subtree_reuse_against_absolute_depths():
    """One small game (stand-in nets, 40 playouts a move, n_thr = 2) under the negamax rule.  Every backup is logged as
    (the path's nodes, the root's ply, the leaf value).  After update_with_move the kept subtree's (n, Q) are what they
    were; and at the end every node still reachable has the (n, Q) that a from-scratch recomputation gives it from the
    log by ABSOLUTE plies alone -- a node at ply D, a playout whose leaf is at ply DL: -lv where DL - D is even, +lv
    where it is odd -- whatever the root was when the playout ran."""
    nets = StandIn(5)
    log = []
    ply = [0]

    def logged(self, leaf_value):
        path, node = [], self
        while node is not None:
            path.append(node)
            node = node.parent
        log.append((path, ply[0], leaf_value))     # (path[-1] is the root of the moment, at ply ply[0])
        negamax_ref.update_recursive(self, leaf_value)

    reference = mcts_py.Node.update_recursive
    mcts_py.Node.update_recursive = logged
    try:
        m = mcts_py.MCTS(nets.policy_fn, nets.value_fn, _rollouts(9), lmbda=0.5, c_puct=1.0, n_thr=2)
        state, color = orc.initial_state(), 1
        for turn in range(6):
            acts = orc.legal_actions(state, color)
            a = m.get_move(state, color, 40) if len(acts) > 0 else -1
            kept = []
            if a in m.root.children:
                _walk(m.root.children[a], 0, kept)
            before = [(n.n_visits, n.Q) for n, _ in kept]
            m.update_with_move(a)
            assert [(n.n_visits, n.Q) for n, _ in kept] == before and (not kept or m.root is kept[0][0])
            if a >= 0:
                orc.place_stone(state, a, color)
            color = 3 - color
            ply[0] += 1
        m.get_move(state, color, 40)
    finally:
        mcts_py.Node.update_recursive = reference
    # from scratch, by absolute plies
    book, at = {}, {}
    for path, root_ply, lv in log:
        leaf_ply = root_ply + len(path) - 1
        for i, node in enumerate(path):
            d = leaf_ply - i
            assert at.setdefault(id(node), d) == d
            n, q = book.get(id(node), (0, 0))
            v = -lv if (leaf_ply - d) % 2 == 0 else lv
            book[id(node)] = (n + 1, q + (v - q) / (n + 1))
    live = []
    _walk(m.root, ply[0], live)
    assert len(live) > 20 and m.root.n_visits > 40          # (the last search carried on from a kept subtree)
    for node, d in live:
        if node.n_visits:
            assert at[id(node)] == d
            assert book[id(node)] == (node.n_visits, node.Q)
        else:
            assert id(node) not in book


def test_backup_arg():
    """Fails on a tree without the feature: engine.backup_arg does not exist there."""
    from iago_amd import engine
    assert engine.backup_arg("reference") == "reference" and engine.backup_arg("negamax") == "negamax"
    for bad in (None, "", "Negamax", "minimax", b"negamax", 0, 1, True, ("negamax",)):
        with pytest.raises(ValueError):
            engine.backup_arg(bad)


@pytest.mark.parametrize("kw", [dict(backup="minimax"), dict(backup=None), dict(backup="negamax", persistent=False),
                                dict(backup="negamax", use_graph=True), dict(backup="negamax", async_steps=True),
                                dict(backup="negamax", lookahead=4)])
def test_engine_refuses_before_it_allocates(kw):
    """A bad string, or "negamax" with the per-playout launches asked for: ValueError before anything is allocated (no
    device is touched: this runs without one)."""
    from iago_amd import engine
    with pytest.raises(ValueError, match="backup"):
        engine.BatchedMCTS(1, None, None, None, **kw)


def test_flag_and_bindings():
    """The flag is the header's, beside the chain-skip flag and apart from it."""
    import os
    import re
    from iago_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "iago_hip_serving.h")).read()
    assert int(re.search(r"#define IAGO_SEARCH_NEGAMAX (0x[0-9a-fA-F]+)", text).group(1), 16) == _lib.SEARCH_NEGAMAX == 0x200
    assert _lib.SEARCH_NEGAMAX & _lib.SEARCH_CHAIN_SKIP == 0
    assert _lib.SEARCH_GAMES_PER_WORKGROUP < min(_lib.SEARCH_NEGAMAX, _lib.SEARCH_CHAIN_SKIP)


@pytest.mark.parametrize("gpw,refused", [(7 | 0x200, True), (7 | 0x300, True), (8 | 0x200, False), (32 | 0x300, False),
                                         (0x200, False), (16 | 0x100, False)])
def test_library_strips_both_flags(gpw, refused):
    """check_args reads games_per_workgroup without BOTH flags: 7 is refused by name whatever flags it carries, 8 / 32 / 0
    (= 32) pass that check with either flag or both (and are refused later: these argument sets cannot be launched)."""
    from tests.test_search_refusals_cpu import Call
    c = Call("persistent")
    c.a.games_per_workgroup = gpw
    rc, msg = c()
    assert rc != 0
    assert (b"games_per_workgroup is 0 (= 32), 8, 16 or 32" in msg) == refused, msg


def test_a_rollout_hook_on_a_negamax_engine_is_refused():
    """A hook is set after construction and selects the per-playout launches, whose backup is the reference's: search()
    refuses on its first line (an engine's shell is enough to see it: nothing else of it is read), as the games' entry
    points do through the same check.  Without a hook, or under the reference's rule, the check passes."""
    from iago_amd import engine
    m = engine.BatchedMCTS.__new__(engine.BatchedMCTS)
    m.backup, m.persistent, m.rollout_hook = "negamax", True, (lambda e: None)
    with pytest.raises(ValueError, match="negamax"):
        m._backup_check()
    with pytest.raises(ValueError, match="negamax"):
        m.search(None, None, None, 10)
    with pytest.raises(ValueError, match="negamax"):
        engine.SelfPlayEngine._play(types.SimpleNamespace(mcts=m), 10, None, True, engine.NO_RULES)
    m.rollout_hook = None
    m._backup_check()
    m.backup, m.rollout_hook = "reference", (lambda e: None)
    m._backup_check()
