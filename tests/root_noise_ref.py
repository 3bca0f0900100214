"""The rule of the root noise (include/iago_hip_serving.h, iago_mcts_root_noise / iago_mcts_search_noise) in numpy, on the
oracle's Philox (pinned to the Random123 vectors in test_oracle_golden.py), and the oracle's MCTS with the mix hooked in at
the root.  At a searched turn t (the game's turn counter, passes included) of the game with global id G whose mover has
the K legal cells `acts` (ascending):

    K < 2   nothing: the counts are 0
    urn     c[a] = 0; for j = 0 .. N-1: weight[a] = alpha_256 + 256 c[a] on the legal cells, W = K alpha_256 + 256 j,
            w_j = word j & 3 of Philox4x32-10 on the counter (G, t, j >> 2, 0), key = seed with its high word ^ 0x44495249,
            r = (w_j * W) >> 32, the lowest legal a with sum_{b <= a} weight[b] > r gets c[a] += 1
    mix     p <- float32(float32(p * keep) + term), keep = float32((256 - eps_256) / 256),
            term = float32(eps_256 * c[a]) * 2^-(8 + log2 N)                       (both exact in float32)

The mix is applied once per searched turn to the root's children: at the turn's start to the children it has, else in the
expansion that creates them (NoisyMCTS)."""
import numpy as np

from oracle import mcts_py
from oracle import oracle as orc

NOISE_KEY = 0x44495249   # "DIRI"
DRAWS = 256


def words(seed, game_id, turn, draws):
    """The urn's `draws` raw 32-bit words of (seed, global game id, turn), in draw order."""
    key = (int(seed) ^ (NOISE_KEY << 32)) & 0xFFFFFFFFFFFFFFFF
    out = []
    for blk in range((draws + 3) // 4):
        out.extend(int(w) for w in orc.philox(key, int(game_id) & 0xFFFFFFFF, int(turn) & 0xFFFFFFFF, blk, 0))
    return out[:draws]


def urn(acts, alpha_256, draws, ws):
    """The counts by cell (int64[64]) of the urn over the legal cells `acts` fed the words ws (draws of them)."""
    acts = sorted(int(a) for a in acts)
    c = np.zeros(64, np.int64)
    if len(acts) < 2:
        return c
    for j in range(draws):
        total = len(acts) * alpha_256 + 256 * j
        r = (int(ws[j]) * total) >> 32
        run = 0
        for a in acts:
            run += alpha_256 + 256 * int(c[a])
            if run > r:
                c[a] += 1
                break
        else:
            raise AssertionError("r >= W")
    return c


def counts(acts, seed, game_id, turn, alpha_256, draws=DRAWS):
    return urn(acts, alpha_256, draws, words(seed, game_id, turn, draws))


def keep_term(c, eps_256, draws):
    lg = int(draws).bit_length() - 1
    assert 1 << lg == draws and 0 <= eps_256 <= 256
    keep = np.float32((256 - eps_256) / 256)
    term = np.float32(np.float32(eps_256 * int(c)) * np.float32(2.0 ** -(8 + lg)))
    assert float(keep) == (256 - eps_256) / 256 and float(term) == eps_256 * int(c) / (256 * draws)   # exact
    return keep, term


def mix(p, c, eps_256, draws=DRAWS):
    """The mixed prior of a stored prior p (float32) whose cell drew c: two float32 roundings."""
    keep, term = keep_term(c, eps_256, draws)
    return np.float32(np.float32(np.float32(p) * keep) + term)


class NoisyMCTS(mcts_py.MCTS):
    """oracle/mcts_py.MCTS with root noise: begin_turn() before every searched turn's get_move draws the turn's counts
    and rewrites the children the root has; playout -- MCTS.playout restated, as tests/wave_mcts.py restates the wave --
    mixes the children of the ROOT when it is the root that expands.  noise = (alpha_256, eps_256, draws)."""

    def __init__(self, *a, noise, seed, game_id, **kw):
        super(NoisyMCTS, self).__init__(*a, **kw)
        self.noise, self.seed, self.game_id = tuple(noise), seed, game_id
        self.counts = None       # the current turn's counts, None: the turn is not noised (K < 2, or a clean turn)
        self.mixed = []          # (test diagnostic) the nodes whose prior the noise rewrote

    def _mix_children(self, node):
        for a, ch in node.children.items():
            ch.P = mix(ch.P, self.counts[a], self.noise[1], self.noise[2])
            ch.u = ch.P
            self.mixed.append(ch)

    def begin_turn(self, state, color, turn, noised=True):
        acts = orc.legal_actions(state, color)
        self.counts = None
        if noised and len(acts) >= 2:
            self.counts = counts(acts, self.seed, self.game_id, turn, self.noise[0], self.noise[2])
            if len(self.root.children) >= 2:
                assert sorted(self.root.children) == sorted(acts)
                self._mix_children(self.root)

    def playout(self, state, color, node):  # MCTS.py:105-133 as oracle/mcts_py.py states it, the mix at the root's expansion
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
            action, node = node.select(self.c_puct)
            state = orc.place_stone(state, action, c)
            c = 3 - c
            depth += 1
