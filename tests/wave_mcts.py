"""The wave search (iago_mcts_search_wave, include/iago_hip_serving.h) restated on top of the oracle's MCTS.py
restatement: W playouts of one tree in flight, steered by in-flight visit counts (vv).

A search of n_sims playouts runs as ceil(n_sims / W) waves (the last one n_sims mod W playouts, or W); playout p is
slot p mod W of wave p div W.  In a wave:
  1. the descents run one after the other in slot order, each oracle.mcts_py.MCTS.playout's descent (expansion when
     the real n_visits >= n_thr, the pass child and single-child cases, the policy net at the expansion, first maximum
     wins) except for the score of child c under parent X: sqrt(X.n + X.vv) in the numerator, c.n + c.vv in the
     denominator and Q_eff = c.Q if c.vv == 0 else (c.Q * c.n - vloss * c.vv) / (c.n + c.vv) in float64 (the float32
     c_puct * P and the float64 sqrt, divide and add as before); a descent that reaches its leaf adds 1 to vv on
     every node of its path, the root included;
  2. every leaf is evaluated as MCTS.playout does (value_fn, rollout_fn in playout order);
  3. the backups run in slot order: vv -= 1 along the path, then the reference's update_recursive.
With W = 1 every vv is 0 at every selection: oracle.mcts_py.MCTS exactly.  TEST INFRASTRUCTURE ONLY.
"""
import math

import numpy as np

from oracle import mcts_py
from oracle import oracle as orc


class WaveNode(mcts_py.Node):

    def __init__(self, parent=None, prob=0):
        super().__init__(parent, prob)
        self.vv = 0   # playouts of the running wave whose path holds this node

    def expand(self, action_probs):
        for action, prob in action_probs:
            if action not in self.children:
                self.children[action] = WaveNode(self, prob)

    def select_wave(self, c_puct, vloss):
        sq = math.sqrt(self.n_visits + self.vv)
        best, best_v = None, None
        for a, ch in self.children.items():
            cp = np.float32(np.float32(c_puct) * ch.P)
            n_c = ch.n_visits + ch.vv
            u = float(cp) * sq / (0.01 + n_c)
            q = float(ch.Q) if ch.vv == 0 else (float(ch.Q) * ch.n_visits - vloss * ch.vv) / n_c
            v = q + u
            if best is None or v > best_v:
                best, best_v = (a, ch), v
        return best


class WaveMCTS(mcts_py.MCTS):
    """oracle.mcts_py.MCTS with W playouts per wave; vloss as the float32 the library is handed."""

    def __init__(self, policy_fn, value_fn, rollout_fn, lmbda=0.5, c_puct=1, n_thr=15, wave=1, vloss=1.0):
        super().__init__(policy_fn, value_fn, rollout_fn, lmbda=lmbda, c_puct=c_puct, n_thr=n_thr)
        self.root = WaveNode(None, 1.0)
        self.wave = int(wave)
        self.vloss = float(np.float32(vloss))

    def descend(self, state, color, node):
        """One descent to its leaf: (the path from the root, the leaf's position, the colour to move there)."""
        c = color
        path = [node]
        while True:
            if node.is_leaf():
                if node.n_visits >= self.n_thr:
                    actions = orc.legal_actions(state, c)
                    if len(actions) < 1:
                        node.children[-1] = WaveNode(node, 1)
                    if len(actions) == 1:
                        node.children[actions[0]] = WaveNode(node, 1)
                    else:
                        prob = np.asarray(self.policy_fn(orc.make_state_var(state, c)), np.float32).reshape(64)
                        self.n_policy_evals += 1
                        node.expand([(a, prob[a]) for a in actions])
                    continue
                return path, state, c
            action, node = node.select_wave(self.c_puct, self.vloss)
            state = orc.place_stone(state, action, c)
            c = 3 - c
            path.append(node)

    def evaluate(self, state, c):
        v = np.float32(self.value_fn(orc.make_state_var(state, c))) if self.lmbda < 1 else 0
        z = self.rollout_fn(state, c) if self.lmbda > 0 else 0
        return (1 - self.lmbda) * v + self.lmbda * z

    def wave_playouts(self, state, color, m):
        slots = []
        for _ in range(m):
            path, s, c = self.descend(np.array(state, dtype=np.float32), color, self.root)
            for nd in path:
                nd.vv += 1
            slots.append((path, s, c))
        values = [self.evaluate(s, c) for path, s, c in slots]
        for (path, _, _), lv in zip(slots, values):
            for nd in path:
                nd.vv -= 1
            path[-1].update_recursive(lv)
            self.n_leaf_evals += 1
            self.max_path = max(self.max_path, len(path))

    def get_move(self, state, color, n_sims):
        done = 0
        while done < n_sims:
            m = min(self.wave, n_sims - done)
            self.wave_playouts(state, color, m)
            done += m
        best, best_n = None, None
        for a, ch in self.root.children.items():
            if best is None or ch.n_visits > best_n:
                best, best_n = a, ch.n_visits
        return best

    def update_with_move(self, last_move):
        if last_move in self.root.children:
            self.root = self.root.children[last_move]
            self.root.parent = None
        else:
            self.root = WaveNode(None, 1.0)


def all_vv(node):
    """Every node's vv, depth first (a finished search leaves them all 0)."""
    out = [node.vv]
    for ch in node.children.values():
        out += all_vv(ch)
    return out
