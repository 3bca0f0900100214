"""The rule of the Gumbel root search (include/iago_hip_serving.h, iago_mcts_gumbel_draw / iago_mcts_search_gumbel /
iago_mcts_gumbel_finish; engine.gumbel_targets) in numpy and python integers, on the oracle's Philox (pinned to the
Random123 vectors in test_oracle_golden.py), and the oracle's MCTS with the rule hooked in at the root.  It imports no
device: the two tables are ops.gumbel_tables()'s, passed in as arrays (gumbel_q16 int32[65536], ln_q16 int32[4096]).

    draw      g[a] = gumbel_q16[c0 >> 16], c0 word 0 of Philox4x32-10 on (G, t, a, 0), key = seed with its high word ^ 0x47554D42
    logit     logit_q16(p) = (e - 127) * 45426 + ln_q16[f >> 11] of the float32 p's biased exponent e and mantissa f
    schedule  row k of sched[m + 1][n_sims]: rows 0, 1 count 0, 1, 2, ...; k >= 2: k counters at 0, L = ceil(log2 k), cur = k;
              until full: extra = max(1, n_sims // (L cur)) times (write the first cur counters, add one to each); cur =
              max(2, cur // 2)
    select    at the ROOT of the search with K >= 2 children: t = sum n, maxN = max n, want = sched[min(m, K)][min(t, n_sims -
              1)]; among the children with n == want (none: with n == maxN) the first maximum of
              g[a] + logit_q16(P) + (((c_visit + maxN) * c_scale_256 * q16) >> 8), q16 = rint(Q * 32768) + 32768 (n > 0), 0 (n == 0)
    move      among the children with n == maxN the first maximum of the same score; one child: that child
    rows      by cell: n, q (0 where unvisited), logit_q16 (INT32_MIN off the children)
    target    softmax(logit / 65536 + sigma(completed q^)) over the legal moves, in float64 (targets)

GumbelMCTS restates MCTS.playout with Node.select replaced at the root, as forced_ref.ForcedMCTS does.  It runs under
negamax_ref.rule() and selection_ref.rule(): a root child's Q is the root mover's value, its stored P the policy's p."""
import numpy as np

from oracle import mcts_py
from oracle import oracle as orc

GUMBEL_KEY = 0x47554D42   # "GUMB"
LN2_Q16 = 45426
C_VISIT = 50
INT32_MIN = -(1 << 31)


def schedule_row(k, n_sims):
    """The sequence of considered visit counts for k considered moves and a budget of n_sims, n_sims entries."""
    if k < 2:
        return list(range(n_sims))
    levels = 0
    while (1 << levels) < k:
        levels += 1
    counters, cur, row = [0] * k, k, []
    while len(row) < n_sims:
        extra = max(1, n_sims // (levels * cur))
        for _ in range(extra):
            row += counters[:cur]
            for i in range(cur):
                counters[i] += 1
        cur = max(2, cur // 2)
    return row[:n_sims]


def schedule(m, n_sims):
    return np.array([schedule_row(k, n_sims) for k in range(m + 1)], np.int16)


def draw(seed, game_id, turn, gumbel_q16):
    """g by cell (int64[64]) of turn `turn` of the game with global id game_id."""
    key = (int(seed) ^ (GUMBEL_KEY << 32)) & 0xFFFFFFFFFFFFFFFF
    out = np.zeros(64, np.int64)
    for a in range(64):
        w = int(orc.philox(key, int(game_id) & 0xFFFFFFFF, int(turn) & 0xFFFFFFFF, a, 0)[0])
        out[a] = int(gumbel_q16[w >> 16])
    return out


def logit_q16(p, ln_q16):
    b = int(np.float32(p).view(np.uint32))
    return (((b >> 23) & 0xFF) - 127) * LN2_Q16 + int(ln_q16[(b & 0x7FFFFF) >> 11])


def q16(q, n):
    if int(n) <= 0:
        return 0
    return int(np.rint(np.float32(np.float32(q) * np.float32(32768.0)))) + 32768


def score(g, logit, q_16, max_n, c_visit, c_scale_256):
    return int(g) + int(logit) + (((int(c_visit) + int(max_n)) * int(c_scale_256) * int(q_16)) >> 8)


def child_score(ch, g, ln_q16, max_n, c_visit, c_scale_256):
    """ch = (action, n, P, Q)."""
    a, n, p, q = ch
    return score(g[a], logit_q16(p, ln_q16), q16(q, n), max_n, c_visit, c_scale_256)


def select(children, g, ln_q16, sched, m, n_sims, c_visit, c_scale_256):
    """The index of the selected child of a root with K >= 2 children [(action, n, P, Q)] in child order."""
    ns = [int(ch[1]) for ch in children]
    t, max_n = sum(ns), max(ns)
    want = int(sched[min(m, len(children))][min(t, n_sims - 1)])
    if want not in ns:
        want = max_n
    best, best_v = None, None
    for i, ch in enumerate(children):
        if ns[i] != want:
            continue
        v = child_score(ch, g, ln_q16, max_n, c_visit, c_scale_256)
        if best is None or v > best_v:
            best, best_v = i, v
    return best


def move(children, g, ln_q16, c_visit, c_scale_256):
    """The move of a searched root: -2 without children, the one child's action, else the survivor."""
    if not children:
        return -2
    if len(children) == 1:
        return int(children[0][0])
    max_n = max(int(ch[1]) for ch in children)
    best, best_v = None, None
    for ch in children:
        if int(ch[1]) != max_n:
            continue
        v = child_score(ch, g, ln_q16, max_n, c_visit, c_scale_256)
        if best is None or v > best_v:
            best, best_v = int(ch[0]), v
    return best


def rows(children, ln_q16):
    """(n int64[64], q float32[64], logit int64[64]) of a root's children [(action, n, P, Q)]."""
    n, q, lg = np.zeros(64, np.int64), np.zeros(64, np.float32), np.full(64, INT32_MIN, np.int64)
    for a, cn, p, cq in children:
        if a >= 0:
            n[a] = int(cn)
            q[a] = np.float32(cq) if int(cn) > 0 else np.float32(0)
            lg[a] = logit_q16(p, ln_q16)
    return n, q, lg


def target_float(n, q, logit, c_visit=C_VISIT, c_scale_256=256):
    """The improved policy of one root in float64 (64 numbers, 0 off the legal moves)."""
    n, q, logit = np.asarray(n, np.float64), np.asarray(q, np.float64), np.asarray(logit, np.int64)
    legal = logit != INT32_MIN
    out = np.zeros(64, np.float64)
    if not legal.any():
        return out
    lg = np.where(legal, logit.astype(np.float64) / 65536.0, 0.0)
    visited = legal & (n > 0)
    x = lg.copy()
    if visited.any():
        p = np.where(visited, np.exp(lg), 0.0)
        big_n = n.sum()
        wq = (p * q).sum() / p.sum()
        v_mix = (wq + big_n * wq) / (1.0 + big_n)
        q_hat = (np.where(visited, q, v_mix) + 1.0) / 2.0
        x = lg + (float(c_visit) + n.max()) * (float(c_scale_256) / 256.0) * q_hat
    x = np.where(legal, x, -np.inf)
    e = np.where(legal, np.exp(x - x.max()), 0.0)
    return e / e.sum()


def targets(n, q, logit, c_visit=C_VISIT, c_scale_256=256, scale=65536, margin=1e-9):
    """(rows int64 (B, 64) = rint(scale pi'), clear bool (B,)): clear[b] says that no cell of row b lies within `margin` of a
    rounding boundary, so that any correct float64 evaluation rounds every cell of the row the same way."""
    n, q, logit = np.atleast_2d(n), np.atleast_2d(q), np.atleast_2d(logit)
    out = np.zeros(n.shape, np.int64)
    clear = np.zeros(n.shape[0], bool)
    for b in range(n.shape[0]):
        x = float(scale) * target_float(n[b], q[b], logit[b], c_visit, c_scale_256)
        out[b] = np.rint(x).astype(np.int64)
        clear[b] = bool(np.all(np.abs(x - np.floor(x) - 0.5) > margin))
    return out, clear


def root_children(node):
    return [(int(a), int(ch.n_visits), ch.P, ch.Q) for a, ch in node.children.items()]


def raw_row(node):
    row = np.zeros(64, np.int64)
    for a, ch in node.children.items():
        if a >= 0:
            row[a] = ch.n_visits
    return row


class GumbelMCTS(mcts_py.MCTS):
    """oracle/mcts_py.MCTS with the Gumbel rule at the root: gumbel = (m, c_scale_256, c_visit), tables = (gumbel_q16,
    ln_q16).  begin_turn(turn, on=True) before every searched turn's get_move: a FRESH root and the turn's draw (on=False: a
    plain turn -- a fast turn of the playout cap -- on the tree as it stands, get_move the most visited child).  get_move
    returns the halving's survivor; rows() / raw_row() afterwards."""

    def __init__(self, *a, gumbel, tables, seed, game_id, **kw):
        super(GumbelMCTS, self).__init__(*a, **kw)
        self.m, self.c_scale_256, self.c_visit = (int(v) for v in gumbel)
        self.gumbel_q16, self.ln_q16 = tables
        self.seed, self.game_id = seed, game_id
        self.on, self.g, self.sched, self.n_sims = False, None, None, 0
        self.picks = []          # (test diagnostic) the root's selections of the current turn, by action
        self.fallbacks = 0       # (test diagnostic) root selections that found no child with the schedule's count

    def begin_turn(self, turn, on=True):
        self.on = bool(on)
        self.picks = []
        if self.on:
            self.root = mcts_py.Node(None, 1.0)
            self.g = draw(self.seed, self.game_id, turn, self.gumbel_q16)

    def select(self, node):
        if not (node is self.root and self.on and len(node.children) >= 2):
            return node.select(self.c_puct)
        ch = root_children(node)
        ns = [c[1] for c in ch]
        want = int(self.sched[min(self.m, len(ch))][min(sum(ns), self.n_sims - 1)])
        self.fallbacks += want not in ns
        i = select(ch, self.g, self.ln_q16, self.sched, self.m, self.n_sims, self.c_visit, self.c_scale_256)
        a = ch[i][0]
        self.picks.append(a)
        return a, node.children[a]

    def playout(self, state, color, node):  # MCTS.playout (oracle/mcts_py.py) with self.select(node) for node.select(c_puct)
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

    def get_move(self, state, color, n_sims):
        if not self.on:
            return super(GumbelMCTS, self).get_move(state, color, n_sims)
        self.n_sims = int(n_sims)
        self.sched = schedule(self.m, self.n_sims)
        for _ in range(n_sims):
            self.playout(np.array(state, dtype=np.float32), color, self.root)
        best = move(root_children(self.root), self.g, self.ln_q16, self.c_visit, self.c_scale_256)
        return None if best == -2 else best

    def rows(self):
        return rows(root_children(self.root), self.ln_q16)

    def raw_row(self):
        return raw_row(self.root)
