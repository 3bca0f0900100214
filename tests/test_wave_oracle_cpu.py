"""The wave search's restatement (tests/wave_mcts.py) on CPU stand-in nets: at W = 1 it IS the oracle's MCTS.py
restatement, tree for tree; at W > 1 a run is a pure function of its inputs and leaves no playout in flight."""
import numpy as np
import pytest

from oracle import mcts_py
from oracle import oracle as orc
from tests.test_oracle_golden import _cmp_tree
from tests.wave_mcts import WaveMCTS, all_vv


class StandIn(object):
    """Deterministic stand-in nets: a fixed linear policy (softmax) and value (tanh) of the planes."""

    def __init__(self, seed):
        rs = np.random.RandomState(seed)
        self.wp = rs.standard_normal((128, 64)).astype(np.float32)
        self.wv = (0.1 * rs.standard_normal(128)).astype(np.float32)

    def policy_fn(self, x):
        logits = np.asarray(x, np.float32).reshape(128) @ self.wp
        e = np.exp(logits - logits.max())
        return (e / e.sum()).astype(np.float32)

    def value_fn(self, x):
        return np.float32(np.tanh(np.asarray(x, np.float32).reshape(128) @ self.wv))


def _rollouts(seed):
    rs = np.random.RandomState(seed)
    return lambda state, c: int(rs.randint(-1, 2))


def _play(make, n_sims, second):
    """A search from the start position, the most visited move, update_with_move, a second search."""
    m = make()
    s = orc.initial_state()
    a = m.get_move(s, 1, n_sims)
    m.update_with_move(a)
    orc.place_stone(s, a, 1)
    b = m.get_move(s, 2, second)
    return m, a, b


@pytest.mark.parametrize("n_thr,n_sims", [(3, 60), (15, 100)])
def test_wave_one_is_the_oracle(n_thr, n_sims):
    nets = StandIn(7)
    ref, a0, b0 = _play(lambda: mcts_py.MCTS(nets.policy_fn, nets.value_fn, _rollouts(3), lmbda=0.5, c_puct=1.0,
                                             n_thr=n_thr), n_sims, 37)
    got, a1, b1 = _play(lambda: WaveMCTS(nets.policy_fn, nets.value_fn, _rollouts(3), lmbda=0.5, c_puct=1.0,
                                         n_thr=n_thr, wave=1, vloss=1.0), n_sims, 37)
    assert (a0, b0) == (a1, b1)
    _cmp_tree(mcts_py.dump_tree(got.root, max_depth=64), mcts_py.dump_tree(ref.root, max_depth=64), "w1")
    assert got.n_leaf_evals == ref.n_leaf_evals and got.n_policy_evals == ref.n_policy_evals


@pytest.mark.parametrize("wave,vloss", [(8, 1.0), (32, 1.0), (32, 0.0), (16, 0.5)])
def test_wave_deterministic_and_vv_zero(wave, vloss):
    nets = StandIn(11)

    def make():
        return WaveMCTS(nets.policy_fn, nets.value_fn, _rollouts(5), lmbda=0.5, c_puct=1.0, n_thr=3, wave=wave,
                        vloss=vloss)
    m1, a1, b1 = _play(make, 100, 37)
    m2, a2, b2 = _play(make, 100, 37)
    assert (a1, b1) == (a2, b2)
    _cmp_tree(mcts_py.dump_tree(m1.root, max_depth=64), mcts_py.dump_tree(m2.root, max_depth=64), "rerun")
    assert set(all_vv(m1.root)) == {0}
    assert m1.root.n_visits >= 37 and m1.n_leaf_evals == 137


def test_wave_changes_the_search():
    """At W > 1 the in-flight visits steer the descents apart: not the W = 1 tree (so the GPU comparisons at W > 1
    pin something W = 1 does not)."""
    nets = StandIn(11)
    trees = []
    for wave in (1, 32):
        m = WaveMCTS(nets.policy_fn, nets.value_fn, _rollouts(5), lmbda=0.5, c_puct=1.0, n_thr=3, wave=wave)
        m.get_move(orc.initial_state(), 1, 64)
        trees.append(mcts_py.dump_tree(m.root, max_depth=64))
    assert trees[0] != trees[1]


def test_wave_entry_point_and_refusals():
    """include/iago_hip_serving.h: its own symbol list, disjoint from the other three; the library refuses bad widths,
    bad virtual losses and whole games before it touches a device."""
    import ctypes as C
    import os
    import re
    from iago_amd import _lib, build
    build.build()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "iago_hip_serving.h")).read()
    assert sorted(set(re.findall(r"IAGO_API[^;(]*?\b(iago_\w+)\s*\(", text))) == sorted(_lib.SERVING_SYMBOLS)
    others = set(_lib.SYMBOLS) | set(_lib.LAYER_SYMBOLS) | set(_lib.EXPERIMENTAL_SYMBOLS)
    assert not others & set(_lib.SERVING_SYMBOLS)
    L = _lib.lib()
    a = _lib.MctsSearchArgs()
    for width, vloss, max_turns in ((4, 1.0, 0), (0, 1.0, 0), (64, 1.0, 0), (8, -1.0, 0), (8, float("nan"), 0),
                                    (8, 1.0, 10), (32, 0.0, 1)):
        w = _lib.SearchWaveArgs()
        w.width, w.vloss = width, vloss
        a.max_turns = max_turns
        assert L.iago_mcts_search_wave(C.byref(a), C.byref(w), None) == -1   # IAGO_ERR_INVALID
    assert L.iago_mcts_search_wave(C.byref(a), None, None) == -1


@pytest.mark.parametrize("wave", [0, 2, 4, 64, True, 8.5])
def test_engine_refuses_bad_waves(wave):
    from iago_amd import engine
    with pytest.raises(ValueError):
        engine.BatchedMCTS(1, None, None, None, wave=wave)
