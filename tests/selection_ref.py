"""The AlphaZero selection rule (include/iago_hip_serving.h, IAGO_SEARCH_PUCT_AZ; engine.BatchedMCTS(selection="alphazero"))
as a replacement for what oracle.mcts_py.Node stores and scores.  TEST INFRASTRUCTURE ONLY.

Two changes and no others:

    stored prior   a node with a parent stores float32(prob); a node without one (MCTS's Node(None, 1.0), at a game's start
                   and after a move that is no child of the root) keeps float32(float32(prob) + float32(0.1)).  A root
                   reached by update_with_move is a former child: it keeps what it stored
    score          Q + float64(float32(c_puct * P)) * sqrt(N_parent) / (1.0 + n); the wave search's denominator is
                   1.0 + n + vv, its Q_eff unchanged.  The first maximum wins

Every restatement the tests have creates its nodes through Node.__init__ and scores through Node.U -- oracle.mcts_py.MCTS,
tests/root_noise_ref.NoisyMCTS (the mix reads the stored P), tests/forced_ref.ForcedMCTS (forced() reads the stored P,
select() calls Node.U) -- but for two copies of the score with 0.01 written out: tests/wave_mcts.WaveNode.select_wave and
tests/forced_ref.puct_score (the pruning's).  The block rebinds all four:

    with selection_ref.rule():
        ... any of those searches, prune_row included ...

(restored when the block ends, however it ends).  It composes with negamax_ref.rule(), which rebinds update_recursive
alone."""
import contextlib
import math

import numpy as np

from oracle import mcts_py
from tests import forced_ref, wave_mcts

VISIT_OFF = 1.0


def node_init(self, parent=None, prob=0):
    """Node.__init__ (oracle/mcts_py.py) with the rule's stored prior."""
    self.parent = parent
    self.children = {}
    self.n_visits = 0
    self.Q = 0
    if parent is None:
        self.P = np.float32(np.float32(prob) + np.float32(0.1))
    else:
        self.P = np.float32(prob)
    self.u = self.P


def node_u(self, c_puct):
    cp = np.float32(np.float32(c_puct) * self.P)
    return float(cp) * math.sqrt(self.parent.n_visits) / (VISIT_OFF + self.n_visits)


def puct_score(c_puct, p, q, n, sq):
    """forced_ref.puct_score (the pruning's score) with the rule's denominator."""
    cp = np.float32(np.float32(c_puct) * np.float32(p))
    return float(q) + float(cp) * sq / (VISIT_OFF + int(n))


def select_wave(self, c_puct, vloss):
    """wave_mcts.WaveNode.select_wave with the rule's denominator."""
    sq = math.sqrt(self.n_visits + self.vv)
    best, best_v = None, None
    for a, ch in self.children.items():
        cp = np.float32(np.float32(c_puct) * ch.P)
        n_c = ch.n_visits + ch.vv
        u = float(cp) * sq / (VISIT_OFF + n_c)
        q = float(ch.Q) if ch.vv == 0 else (float(ch.Q) * ch.n_visits - vloss * ch.vv) / n_c
        v = q + u
        if best is None or v > best_v:
            best, best_v = (a, ch), v
    return best


@contextlib.contextmanager
def rule():
    """The oracle's nodes store and score by the AlphaZero rule inside the block."""
    saved = (mcts_py.Node.__init__, mcts_py.Node.U, wave_mcts.WaveNode.select_wave, forced_ref.puct_score)
    mcts_py.Node.__init__ = node_init
    mcts_py.Node.U = node_u
    wave_mcts.WaveNode.select_wave = select_wave
    forced_ref.puct_score = puct_score
    try:
        yield
    finally:
        mcts_py.Node.__init__, mcts_py.Node.U, wave_mcts.WaveNode.select_wave, forced_ref.puct_score = saved
