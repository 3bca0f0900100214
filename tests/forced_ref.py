"""The rule of forced playouts and policy-target pruning (include/iago_hip_serving.h, iago_mcts_search_forced /
iago_mcts_prune_visits) in numpy and python floats, hooked into the oracle's MCTS with root noise (tests/root_noise_ref.py).
k = k_256 / 256, k_256 an integer in 1 .. 4096:

    forced(n, p, N)   n >= 1 and float64(256 n n) < (float64(k_256) * float64(p)) * float64(N)
                      n a child's visits, p its stored float32 prior (after the + 0.1 and the turn's mix), N the root's
                      visits; the left side and the first product are exact, the second product rounds once
    select            at the ROOT of the search, K >= 2 children: a forced child scores +inf, the others Q + u; first maximum
    prune             b = the first child with the most visits, S* = its score under sq = sqrt(N); every other child c with
                      n >= 1: F = #{j in 1 .. n - 1: forced(j, p_c, N)}; m = n; while n - m < F and score(c with m - 1
                      visits) < S*: m -= 1; m = 0 if m < n and m == 1.  Fewer than two children: the raw row

ForcedMCTS restates NoisyMCTS.playout with Node.select replaced at the root, as root_noise_ref restates MCTS.playout."""
import math

import numpy as np

from oracle import mcts_py
from oracle import oracle as orc
from tests import root_noise_ref as rn

INF = float("inf")


def forced(n, p, N, k_256):
    n, N = int(n), int(N)
    kp = float(int(k_256)) * float(np.float32(p))          # 12 x 24 bits: exact
    assert n < (1 << 22)                                    # 256 n n is exact
    return n >= 1 and float(256 * n * n) < kp * float(N)


def puct_score(c_puct, p, q, n, sq):
    """Node.get_value as oracle/mcts_py.Node.select computes it: float32 c_puct * P, then float64."""
    cp = np.float32(np.float32(c_puct) * np.float32(p))
    return float(q) + float(cp) * sq / (0.01 + int(n))


def prune_row(children, N, c_puct, k_256):
    """children: the root's (action, n, P, Q) in child order; N: the root's visits.  The pruned visit row, int64[64]."""
    row = np.zeros(64, np.int64)
    for a, n, _, _ in children:
        if a >= 0:
            row[a] = n
    if len(children) < 2:
        return row
    b = 0
    for i, ch in enumerate(children):                      # the first maximum (MCTS.py:147)
        if ch[1] > children[b][1]:
            b = i
    sq = math.sqrt(int(N))
    s_star = puct_score(c_puct, children[b][2], children[b][3], children[b][1], sq)
    for i, (a, n, p, q) in enumerate(children):
        if i == b or n < 1:
            continue
        f = sum(1 for j in range(1, n) if forced(j, p, N, k_256))
        m = n
        while n - m < f and puct_score(c_puct, p, q, m - 1, sq) < s_star:
            m -= 1
        if m < n and m == 1:
            m = 0
        row[a] = m
    return row


def root_children(node):
    return [(int(a), int(ch.n_visits), ch.P, ch.Q) for a, ch in node.children.items()]


def raw_row(node):
    row = np.zeros(64, np.int64)
    for a, ch in node.children.items():
        if a >= 0:
            row[a] = ch.n_visits
    return row


class ForcedMCTS(rn.NoisyMCTS):
    """root_noise_ref.NoisyMCTS with forced playouts: k_256 (None or 0: NoisyMCTS itself).  begin_turn(..., noised=)
    switches the forcing with the noise (a clean turn of the playout cap is not forced); pruned_row() after get_move."""

    def __init__(self, *a, k_256=None, **kw):
        super(ForcedMCTS, self).__init__(*a, **kw)
        self.k_256 = int(k_256 or 0)
        self.forcing = True
        self.n_forced = 0        # (test diagnostic) selections a forced child won

    def begin_turn(self, state, color, turn, noised=True):
        super(ForcedMCTS, self).begin_turn(state, color, turn, noised=noised)
        self.forcing = bool(noised)

    def select(self, node):      # Node.select (oracle/mcts_py.py) with the +inf at the root of the search
        force = node is self.root and self.forcing and self.k_256 > 0 and len(node.children) >= 2
        best, best_v = None, None
        for a, ch in node.children.items():
            ch.u = ch.U(self.c_puct)
            v = float(ch.Q) + ch.u
            if force and forced(ch.n_visits, ch.P, node.n_visits, self.k_256):
                v = INF
            if best is None or v > best_v:
                best, best_v = (a, ch), v
        self.n_forced += best_v == INF
        return best

    def playout(self, state, color, node):  # NoisyMCTS.playout with self.select(node) for node.select(c_puct)
        c = color
        depth = 1
        while True:
            if node.is_leaf():
                if node.n_visits >= self.n_thr:
                    actions = orc.legal_actions(state, c)
                    if len(actions) < 1:
                        node.children[-1] = mcts_py.Node(node, 1)
                    if len(actions) == 1:
                        node.children[actions[0]] = mcts_py.Node(node, 1)
                    else:
                        prob = np.asarray(self.policy_fn(orc.make_state_var(state, c)), np.float32).reshape(64)
                        self.n_policy_evals += 1
                        node.expand([(a, prob[a]) for a in actions])
                        if node is self.root and self.counts is not None and len(actions) >= 2:
                            self._mix_children(node)
                    continue
                x = orc.make_state_var(state, c)
                v = np.float32(self.value_fn(x)) if self.lmbda < 1 else 0
                z = self.rollout_fn(state, c) if self.lmbda > 0 else 0
                leaf_value = (1 - self.lmbda) * v + self.lmbda * z
                node.update_recursive(leaf_value)
                self.n_leaf_evals += 1
                self.max_path = max(self.max_path, depth)
                return leaf_value
            action, node = self.select(node)
            state = orc.place_stone(state, action, c)
            c = 3 - c
            depth += 1

    def pruned_row(self):
        return prune_row(root_children(self.root), self.root.n_visits, self.c_puct, self.k_256)
