"""Batched PV-MCTS and self-play on one GPU.

Two engines behind one class, same trees bit for bit: the PERSISTENT search (round 4; the default wherever the
split-f16 Value net and the three-piece SLPolicy apply) -- a whole search, or a whole batch of self-play games, as
ONE launch in which every game runs on its own clock (iago_mcts_search_persistent, csrc/search_kernel.hip) -- and
the per-playout launches described below (use_graph=True and the look-ahead options select them).

Host-side select/expand/backup loop over thousands of games (the reference runs
one game, one playout at a time: MCTS.py:105-147, game.py:117-142).  Every
tree operation, board update and the leaf rollout is a HIP kernel behind the C
ABI (include/iago_hip.h); the policy and value nets are PyTorch-ROCm modules
(or any callables on a CUDA planes tensor).  The reference's constants and
quirks are the defaults: lmbda=0.5, c_puct=1, n_thr=15,
P = prior + 0.1, U = c*P*sqrt(N)/(0.01+n), root evaluated itself for its first
n_thr simulations, no sign flip in backup, pass = action -1, subtree reuse.
The wall-clock budget (10 s per move, MCTS.py:142) becomes a simulation count.
"""
import collections
import ctypes as C
import numbers
import os

import numpy as np
import torch

from . import _lib, ops
from ._lib import MctsTree, check

START_OWN = 0x0000000810000000  # colour 1 "X", moves first: (3,4), (4,3)  (game.py:26-30)
START_OPP = 0x0000001008000000  # colour 2 "O": (3,3), (4,4)
HANDICAP_CELLS = (2 * 8 + 4, 3 * 8 + 5, 4 * 8 + 2, 5 * 8 + 3)  # src/train_rl.py:45
STREAM_REC_BYTES = 4 << 30      # SelfPlayEngine.play_stream: largest rec_pi (n_games x max_turns x 64 int32) it allocates


def _p(t):
    return C.c_void_p(t.data_ptr())


_stream = ops._stream   # the current HIP stream as a void*

# The rules of a batch of games beyond plain PV-MCTS, validated once (_play_rules) and handed on as ONE value:
# solve_empties (None: off, else an int in [0, 20]), explore_turns (an int, 0: off), playout_cap (None: off, else
# (n_fast, full_per_256)), root_noise (None: off, else (alpha_256, eps_256, draws)), forced_playouts (None: off, else k_256,
# with root_noise), solved_targets (False: off; True, with solve_empties: the solved turns record the set of their
# optimal moves), gumbel (None: off, else (m, c_scale_256, c_visit): the Gumbel root search, without root_noise,
# forced_playouts or explore_turns), root_values (False: off; True: every searched turn records its root's value and
# visits, the turn loop) -- as SelfPlayEngine.play documents them.
PlayRules = collections.namedtuple("PlayRules", "solve_empties explore_turns playout_cap root_noise forced_playouts "
                                   "solved_targets gumbel root_values", defaults=(None, None, False, None, False))
NO_RULES = PlayRules(None, 0, None)


# ---- The root rules -------------------------------------------------------------------------------------------------------
# What a search does at its roots: nothing of its own (None: the plain root), root noise with or without forced playouts, or
# the Gumbel root search.  All that differs between them is here ("The root rules").
class RootRule(collections.namedtuple("RootRule", "root_noise forced_playouts gumbel")):
    """A rule as search() takes it, validated (root_rule).  It answers: the engines it is offered for, the step before the
    launch, the launch, the move, the recorded policy target."""
    __slots__ = ()
    fresh = property(lambda self: self.gumbel is not None)   # FRESH roots: search() resets the searched trees, no compaction
    targets = property(lambda self: self.gumbel is not None or self.forced_playouts is not None)   # a target of its own

    def require(self, m):
        """The persistent search only; Gumbel under the negamax backup and the AlphaZero selection.  m None: not asked."""
        if m is not None and self.gumbel is not None and getattr(m, "backup", "reference") != "negamax":
            raise ValueError("gumbel needs backup=\"negamax\" (a root child's Q must be the root mover's value)")
        if m is not None and self.gumbel is not None and getattr(m, "selection", "reference") != "alphazero":
            raise ValueError("gumbel needs selection=\"alphazero\" (a child's stored prior must be the policy's p)")
        if m is not None and (not getattr(m, "persistent", False) or getattr(m, "wave_entry", False)
                              or getattr(m, "rollout_hook", None) is not None or getattr(m, "use_graph", False)
                              or getattr(m, "async_steps", False) or getattr(m, "lookahead", 0)):
            raise ValueError("%s is offered for the persistent search only (not use_graph, async steps, the look-ahead, "
                             "rollout_hook or the wave search)" % ("root_noise" if self.gumbel is None else "gumbel"))
        return self

    def draw(self, m, own, opp, active, turn):
        """Before the launch: the urn of turn `turn` (the counts rows, the mix on the children the roots have), or the draw."""
        if self.gumbel is None:
            ops.root_noise(m.tree.ref(), active, own, opp, m.seed, *m._turn_ids(turn), self.root_noise, m._noise_rows())
        else:
            st = m._gumbel_state()
            ops.gumbel_draw(m.tree.ref(), active, m.seed, *m._turn_ids(turn), self.gumbel, st["tables"], st["g"])

    def launch(self, m, args, n_sims, game=None):
        """The rule's entry point on the engine's split handle; never whole games."""
        if game is not None:
            raise ValueError("whole games in one launch are not available with %s (the turn loop is)"
                             % ("root noise" if self.gumbel is None else "the Gumbel root search"))
        if self.gumbel is not None:
            st = m._gumbel_state()
            ops.search_gumbel(args, self.gumbel, st["tables"], m._gumbel_sched(self.gumbel[0], n_sims), st["g"], streams=m._split)
            st["last"] = self.gumbel
        elif self.forced_playouts is None:
            ops.search_noise(args, self.root_noise, m._noise_rows(), streams=m._split)
        else:
            ops.search_forced(args, self.root_noise, m._noise_rows(), self.forced_playouts, streams=m._split)

    def move(self, m, active, record=False):
        """After the search: the Gumbel root writes the halving's survivor over best_move's in the engine's move buffer and,
        for a recorded game, returns the improved policy of the rows it fills (made now, before the turn's other launches)."""
        if self.gumbel is not None:
            rows = m.gumbel_rows(active, self.gumbel)
            return gumbel_targets(rows, self.gumbel[2], self.gumbel[1]) if record else None

    def target(self, m, active, made):
        """With `targets`, the recorded policy target of the searched games: what move() made, or the pruned visit row."""
        return made if self.gumbel is not None else m.pruned_visits(active, self.forced_playouts)

    @classmethod
    def of(cls, rules):
        """The RootRule of a PlayRules (validated: _play_rules), None: the plain root."""
        root = cls(rules.root_noise, rules.forced_playouts, rules.gumbel)
        return None if root == (None, None, None) else root


def root_rule(n_sims, root_noise=None, forced_playouts=None, gumbel=None, explore_turns=None, beside="", engine=None):
    """The RootRule of search()'s or play()'s arguments (None: the plain root), each refused where its validator refuses
    it, in search()'s order.  The one place that knows what excludes what: gumbel stands alone (explore_turns, `beside`:
    play()'s) and needs n_sims in [1, 32767] (None: no budget yet); forced_playouts needs root_noise.  engine: require()."""
    gz, root = ops.gumbel_arg(gumbel), None
    if gz is not None:
        if root_noise is not None or forced_playouts is not None or ops.explore_turns_arg(explore_turns):
            raise ValueError("gumbel is not available together with %sroot_noise or forced_playouts (the Gumbel root search "
                             "explores by its own draw)" % beside)
        root = RootRule(None, None, gz).require(engine)
        if n_sims is not None and not 1 <= n_sims <= 32767:
            raise ValueError("gumbel: n_sims must be in [1, 32767], not %r" % (n_sims,))
    noise = ops.root_noise_arg(root_noise)
    if noise is not None:
        root = RootRule(noise, None, None).require(engine)
    k_256 = ops.forced_playouts_arg(forced_playouts, noise)
    return root if k_256 is None else root._replace(forced_playouts=k_256)


class AlphaBeta(collections.namedtuple("AlphaBeta", "depth split", defaults=(0,))):
    """The fixed-depth alpha-beta opponent of SelfPlayEngine.play_match(opponent=): ops.alphabeta_moves at `depth` (an
    int in [1, 10]), the outside yardstick that owes nothing to the nets.  split (0, the default: none; 1 or 2, below
    depth): every root's search spread over the lanes (ops.alphabeta_moves(split=)): the same moves."""
    __slots__ = ()

    def __new__(cls, depth, split=0):
        depth = ops.alphabeta_depth_arg(depth)
        return super(AlphaBeta, cls).__new__(cls, depth, ops.alphabeta_split_arg(split, depth))


# The room play_match gives a split launch of n positions, in jobs: n x this, by split.  (1024 random-play positions of
# 20 to 40 empties: at most 22 / 279 jobs for one root, 11 / 130 on average.)  A turn whose jobs do not fit is answered
# by the unsplit launch: the same moves.
ALPHABETA_JOBS_PER_ROOT = {1: 32, 2: 1024}


# a match beyond PV-MCTS against its own policy net, validated by play_match: opponent (None: the policy net, else an
# AlphaBeta), opening_turns (an even int in [0, 16]: the turns both colours play ops.random_moves'), id_mod (the games
# that share an opening: game g draws with id g mod id_mod)
MatchRules = collections.namedtuple("MatchRules", "opponent opening_turns id_mod")


def _read_back(values):
    """The device values of the dict `values` (0-dim tensors or short integer vectors; None: left out) on the host after
    ONE torch.cat(...).tolist() -- one host synchronisation: a dict under the same names, an int for a 0-dim value, a
    list of ints for a vector."""
    values = {k: v for k, v in values.items() if v is not None}
    flat = torch.cat([v.to(torch.int64).reshape(-1) for v in values.values()]).tolist()
    out, at = {}, 0
    for k, v in values.items():
        out[k] = flat[at] if v.dim() == 0 else flat[at:at + v.numel()]
        at += v.numel()
    return out

_SEARCH_STREAMS = {}    # (device, game CUs) -> iago_search_streams* (None: this runtime gives no CU-masked streams)


def _search_streams(game_cus):
    """The process's CU-masked streams of the role-split search on the current device (iago_mcts_search_streams_create:
    created once, kept for the life of the process), or None where they cannot be had."""
    key = (torch.cuda.current_device(), int(game_cus))
    if key not in _SEARCH_STREAMS:
        h = C.c_void_p()
        rc = _lib.lib().iago_mcts_search_streams_create(int(game_cus), C.byref(h))
        _SEARCH_STREAMS[key] = h if rc == 0 and h.value else None
    return _SEARCH_STREAMS[key]


def _split_arg(want):
    """split= / IAGO_SEARCH_SPLIT: "auto", or the game CUs of the role split -- 0 (the single launch) or a positive
    multiple of 8.  Anything else is refused: the widening loop of BatchedMCTS would turn it into a count that is no
    multiple of 8, and the search would quietly take the single launch."""
    if isinstance(want, str):
        if want == "auto":
            return want
        try:
            n = int(want.strip())
        except ValueError:
            n = None
    else:
        n = int(want) if isinstance(want, numbers.Integral) and not isinstance(want, bool) else None
    if n is None or n < 0 or n % 8:
        raise ValueError("split / IAGO_SEARCH_SPLIT: \"auto\", 0 or a positive multiple of 8 (game CUs) expected, not %r"
                         % (want,))
    return n


BACKUP_RULES = ("reference", "negamax")


def backup_arg(x):
    """backup=: the rule by which a playout's leaf value climbs its path -- "reference" (the reference's
    Node.update_recursive: the same value at every level) or "negamax" (the sign turns at every level: a node's Q is the
    value for the player who moved into it; include/iago_hip_serving.h, IAGO_SEARCH_NEGAMAX).  The canonical string, or
    ValueError."""
    if isinstance(x, str) and x in BACKUP_RULES:
        return x
    raise ValueError("backup: \"reference\" or \"negamax\" expected, not %r" % (x,))


_NEGAMAX_NEEDS = ("backup=\"negamax\" is offered for the persistent search only (the per-playout launches -- "
                  "persistent=False, use_graph, the look-ahead, asynchronous steps and what a rollout_hook selects -- keep "
                  "the reference's rule)")


SELECTION_RULES = ("reference", "alphazero")


def selection_arg(x):
    """selection=: the rule by which Node.select scores a child -- "reference" (the reference's: the stored prior is
    prob + 0.1, the exploration term divides by 0.01 + n) or "alphazero" (the textbook rule: the stored prior is prob,
    U = c_puct P sqrt(N) / (1 + n); include/iago_hip_serving.h, IAGO_SEARCH_PUCT_AZ).  The canonical string, or
    ValueError."""
    if isinstance(x, str) and x in SELECTION_RULES:
        return x
    raise ValueError("selection: \"reference\" or \"alphazero\" expected, not %r" % (x,))


_ROOT_VALUE_NEEDS = ("root values need backup=\"negamax\" (under the reference's rule a root's Q mixes both players' views and "
                     "is no value)")


_ALPHAZERO_NEEDS = ("selection=\"alphazero\" is offered for the persistent search only (the per-playout launches -- "
                    "persistent=False, use_graph, the look-ahead, asynchronous steps and what a rollout_hook selects -- keep "
                    "the reference's rule)")


def suggest_capacity(n_sims, n_thr=15, moves=64, branching=12):
    """Nodes per game that a whole self-play game needs without ever compacting the pools:
    every expansion adds ~`branching` children, a search adds at most
    n_sims / n_thr + 1 expansions.  The turn-by-turn loop (BatchedMCTS.search) compacts a pool that is
    half full -- TreePool.compact -- so there a smaller capacity only costs compaction passes, as long as
    one search's live tree fits in half of it.  The one-launch whole-game path of the persistent search
    never compacts: SelfPlayEngine.play takes it only for a pool of at least half this size (the nodes a
    game really leaves behind: 1,718 at 100 playouts per move) and replays the batch through the turn
    loop if a pool fills up all the same."""
    per_move = (n_sims // max(n_thr, 1) + 1) * branching
    cap = 1024
    while cap < per_move * moves:
        cap *= 2
    return cap


class TreePool(object):
    """Device memory of the per-game search trees (iago_mcts_tree): ONE array of 32-byte node
    records (iago_mcts_node); `n_visits`, `q`, `p`, `v`, `first_child`, `parent`, `action`,
    `n_children` are strided views of it (read them with .cpu(), fill them in place)."""

    def __init__(self, n_games, capacity, device="cuda", value_cache=False):
        if not torch.cuda.is_available():
            raise _lib.IagoError("TreePool needs a HIP device (no CPU fallback)")
        self.n_games, self.capacity = n_games, capacity
        self._alloc(device, value_cache)
        self.reset()

    def _alloc(self, device, value_cache):
        n = self.n_games * self.capacity
        kw = dict(device=device)
        self.nodes = torch.zeros((n, _lib.NODE_WORDS), dtype=torch.int32, **kw)
        f32, i8 = self.nodes.view(torch.float32), self.nodes.view(torch.int8)
        self.n_visits, self.q, self.p = self.nodes[:, 0], f32[:, 1], f32[:, 2]
        # value_func(node) once evaluated, NaN before (iago_mcts_fresh_leaves); None = no cache
        self.v = f32[:, 3] if value_cache else None
        self.first_child, self.parent = self.nodes[:, 4], self.nodes[:, 5]
        self.action, self.n_children = i8[:, 24], self.nodes.view(torch.uint8)[:, 25]
        self.n_nodes = torch.zeros(self.n_games, dtype=torch.int32, **kw)
        self.root = torch.zeros(self.n_games, dtype=torch.int32, **kw)
        self.overflow = torch.zeros(self.n_games, dtype=torch.int32, **kw)
        t = MctsTree()
        t.n_games, t.capacity, t.has_v = self.n_games, self.capacity, 1 if value_cache else 0
        t.nodes = self.nodes.data_ptr()
        t.n_nodes, t.root, t.overflow = self.n_nodes.data_ptr(), self.root.data_ptr(), self.overflow.data_ptr()
        self.c = t

    def ref(self):
        return C.byref(self.c)

    def reset(self, mask=None):
        check(_lib.lib().iago_mcts_reset(self.ref(), _p(mask) if mask is not None else None,
                                         _stream()), "iago_mcts_reset")
        for hook in getattr(self, "reset_hooks", ()):
            hook(mask)

    def bytes(self):
        return self.nodes.numel() * 4

    def compact(self, mask=None):
        """Garbage collection (iago_mcts_compact): the live subtree of every game (mask: uint8
        per game, None = all) re-laid from index 0; the nodes abandoned by subtree reuse are
        freed.  A second pool and an index array are allocated on first use."""
        if getattr(self, "_scratch", None) is None:
            sc = TreePool.__new__(TreePool)
            sc.n_games, sc.capacity = self.n_games, self.capacity
            sc._alloc(self.nodes.device, self.v is not None)
            self._scratch = sc
            self._order = torch.empty(self.n_games * self.capacity, dtype=torch.int32, device=self.nodes.device)
        check(_lib.lib().iago_mcts_compact(self.ref(), self._scratch.ref(), _p(self._order),
                                           _p(mask) if mask is not None else None, _stream()),
              "iago_mcts_compact")

    def dump(self, g, max_depth=6):
        """Host copy of game g's tree in the format of oracle.mcts_py.dump_tree."""
        lo, hi = g * self.capacity, g * self.capacity + int(self.n_nodes[g].item())
        rec = self.nodes[lo:hi].cpu()
        f32, i8 = rec.view(torch.float32), rec.view(torch.int8)
        arr = {"first_child": rec[:, 4].numpy(), "n_children": rec.view(torch.uint8)[:, 25].numpy(),
               "action": i8[:, 24].numpy(), "n_visits": rec[:, 0].numpy(), "q": f32[:, 1].numpy(),
               "p": f32[:, 2].numpy()}

        def rec(i, depth):
            d = dict(n=int(arr["n_visits"][i]), Q=float(arr["q"][i]), P=float(arr["p"][i]),
                     children={}, order=[])
            fc, k = int(arr["first_child"][i]), int(arr["n_children"][i])
            if fc >= 0:
                d["order"] = [int(arr["action"][fc + j]) for j in range(k)]
                if depth < max_depth:
                    for j in range(k):
                        d["children"][str(int(arr["action"][fc + j]))] = rec(fc + j, depth + 1)
            return d

        return rec(int(self.root[g].item()), 0)


class BatchedMCTS(object):
    """MCTS(lmbda, c_puct, n_thr) of MCTS.py:78-154 for n_games trees at once.

    policy_fn(planes) -> (L,64) probabilities, value_fn(planes) -> (L,) values,
    planes = (L,2,8,8) float32 CUDA tensor (GameFunctions.make_state_var
    layout).  rollout_weights: ops.RolloutWeights (None = uniform random
    rollouts).  rollout_hook(engine) runs after every rollout launch (tests record `engine.z`).

    Two ways through a playout (MCTS.py:105-133), same trees:
      * sync-free (default when policy_fn has `forward_counted(planes, n_dev)`, as
        network.SLPolicy does): the number of leaves that expand stays on the device
        (iago_mcts_pending -> n_dev of the policy kernels and of iago_mcts_expand), so a
        playout is a fixed sequence of launches with no host synchronisation --
        select, pending, planes, policy net, expand, continue-select, value net, rollout,
        leaf mix + backup.  use_graph=True captures that sequence once and replays it
        with ONE launch per playout.
      * host-counted (arbitrary callables, e.g. the stand-in nets of the parity tests):
        one host sync per playout tells how many leaves expand; the policy callable sees
        exactly those rows.  sync_free=True forces the first way for any callable (it
        is then evaluated on all n_games rows, those past the count being ignored).
    """

    def __init__(self, n_games, policy_fn, value_fn, rollout_weights, lmbda=0.5, c_puct=1.0,
                 n_thr=15, capacity=4096, seed=0, game_id_base=0, device="cuda", use_graph=False,
                 sync_free=None, lookahead=None, lookahead_slots=None, value_cache=None, lookahead_overlap=None,
                 z_log_rows=0, async_steps=None, async_parts=None, value_ahead=None, persistent=None,
                 net_workgroups=None, max_cus=None, split=None, wave=1, virtual_loss=1.0, chain_skip=True,
                 path_stride=None, backup="reference", selection="reference"):
        if n_thr < 1:
            raise ValueError("n_thr must be >= 1")
        # (what the caller asked for explicitly, before the defaults below fill the options in: any of these selects
        # the per-playout launches unless `persistent` says otherwise)
        per_playout_asked = bool(use_graph or async_steps or value_ahead or lookahead is not None
                                 or lookahead_overlap is not None or sync_free is not None)
        env_p = os.environ.get("IAGO_PERSISTENT")

        def schedule(can):
            """The persistent search (True) or the per-playout launches, `can` saying whether the former applies: ON wherever
            it does unless the caller asks for the per-playout launches (a rollout hook comes later); the environment
            variable IAGO_PERSISTENT=0 / 1 overrides both (measurements: tools/time_value_ahead.py)."""
            if env_p in ("0", "1"):
                return can and env_p == "1"
            return can and not per_playout_asked if persistent is None else persistent

        # backup: the backup rule of the persistent search, "reference" (the default: today's trees bit for bit) or
        # "negamax" (IAGO_SEARCH_NEGAMAX; backup_arg).  The per-playout launches have the reference's rule only.  A caller
        # who asks for them and for "negamax" is refused here, before anything is allocated; where the ENGINE takes them
        # (the persistent search does not apply: the nets, the rollout weights, too many games) the refusal comes once that
        # is known, below -- after the tree pool and the state tensors exist, which the exception then frees.  A rollout
        # hook, set after construction, is refused where it would be used (_backup_check)
        self.backup = backup_arg(backup)
        if self.backup == "negamax" and not schedule(True):
            raise ValueError(_NEGAMAX_NEEDS)
        # selection: the selection rule of the persistent search, "reference" (the default: today's trees bit for bit) or
        # "alphazero" (IAGO_SEARCH_PUCT_AZ; selection_arg).  Offered and refused exactly as backup="negamax" is
        self.selection = selection_arg(selection)
        if self.selection == "alphazero" and not schedule(True):
            raise ValueError(_ALPHAZERO_NEEDS)
        # (the persistent search) chain_skip: a descent jumps over the pass chain it remembers from its game's last
        # playout (IAGO_SEARCH_CHAIN_SKIP: timing only, same trees; False: every level is walked -- the A/B switch).
        # path_stride: entries of a game's path buffer (None: 520, the descent's own bound of 512 levels and a margin; at
        # least 8).  A path that does not fit is reported like a full pool; 32 paths that fit a workgroup's LDS live there
        if path_stride is not None and (isinstance(path_stride, bool) or int(path_stride) != path_stride or path_stride < 8):
            raise ValueError("path_stride must be None or an int >= 8, not %r" % (path_stride,))
        self.chain_skip = bool(chain_skip)
        # Wave search (iago_mcts_search_wave in include/iago_hip_serving.h): `wave` playouts of every tree in flight at
        # once, steered by virtual visits (an in-flight visit counts as a loss of `virtual_loss`), descents and backups
        # in slot order -- deterministic, and with wave = 1 today's search bit for bit.  For ONE game (MCTS.get_move)
        # the chip otherwise waits on one playout at a time.  wave > 1 needs the persistent search (its single launch).
        if isinstance(wave, bool) or wave not in (1, 8, 16, 32):
            raise ValueError("wave must be 1, 8, 16 or 32, not %r" % (wave,))
        virtual_loss = float(virtual_loss)
        if not (0.0 <= virtual_loss < float("inf")):
            raise ValueError("virtual_loss must be a finite number >= 0, not %r" % (virtual_loss,))
        self.wave, self.virtual_loss = int(wave), virtual_loss
        self.wave_entry = self.wave > 1   # (True at wave 1 too: the wave entry point at width 1 -- what the tests set)
        ns = n_games * self.wave          # the slots: per-playout state of the search, W per tree
        # (checked before anything is allocated)
        want = _split_arg(split if split is not None else os.environ.get("IAGO_SEARCH_SPLIT", "auto"))
        self.n_games = n_games
        self.policy_fn, self.value_fn, self.rollout_weights = policy_fn, value_fn, rollout_weights
        self.lmbda, self.c_puct, self.n_thr = float(lmbda), float(c_puct), int(n_thr)
        self.seed, self.game_id_base = seed, game_id_base
        kw = dict(device=device)
        # Value cache (iago_mcts_fresh_leaves in include/iago_hip.h): the value net runs only on
        # the leaves it has not evaluated yet (~15 % of the playouts' leaves); every other visit
        # of a leaf takes the value stored in its node.  Same trees.  Default: on whenever the
        # value net can be fed a device-side list of boards.
        can_cache = (value_fn is not None and self.lmbda < 1.0
                     and getattr(value_fn, "forward_boards_counted", None) is not None
                     and getattr(value_fn, "split_f16", False))
        if value_cache is None:
            value_cache = can_cache
        if value_cache and not can_cache:
            raise ValueError("value_cache needs a value net with forward_boards_counted (split-f16 path) and lmbda < 1")
        self.value_cache = bool(value_cache)
        self.tree = TreePool(n_games, capacity, device, value_cache=self.value_cache)
        self._fresh_idx = torch.zeros(n_games, dtype=torch.int64, **kw)
        self._fresh_count = torch.zeros(1, dtype=torch.int32, **kw)
        self._value_total = torch.zeros(1, dtype=torch.int64, **kw)  # value-net evaluations, on the device
        self._value_key = None
        self._vtable = None   # (the persistent search's position table, where it keeps one)
        self._policy_key = None
        self.fused_leaf_eval = os.environ.get("IAGO_FUSED_LEAF_EVAL", "1") != "0"
        self.cur_node = torch.zeros(ns, dtype=torch.int32, **kw)
        self.cur_own = torch.zeros(ns, dtype=torch.int64, **kw)
        self.cur_opp = torch.zeros(ns, dtype=torch.int64, **kw)
        self.needs_expand = torch.zeros(n_games, dtype=torch.uint8, **kw)
        self._pending = torch.zeros(n_games, dtype=torch.uint8, **kw)
        self._pend_idx = torch.zeros(n_games, dtype=torch.int64, **kw)
        self._pend_games = torch.zeros(n_games, dtype=torch.int32, **kw)
        self._pend_count = torch.zeros(1, dtype=torch.int32, **kw)
        self._pend_total = torch.zeros(1, dtype=torch.int64, **kw)  # policy evaluations, on the device
        self.legal = torch.zeros(n_games, dtype=torch.int64, **kw)
        self.leaf_value = torch.zeros(ns, dtype=torch.float32, **kw)
        self.planes = torch.zeros((n_games, 2, 8, 8), dtype=torch.float32, **kw)
        self.z = torch.zeros(ns, dtype=torch.int8, **kw)
        self.v = torch.zeros(n_games, dtype=torch.float32, **kw)
        self.move = torch.zeros(n_games, dtype=torch.int8, **kw)
        self.visits = torch.zeros((n_games, 64), dtype=torch.int32, **kw)
        self._policy_in = torch.zeros((max(n_games, 16), 2, 8, 8), dtype=torch.float32, **kw)
        self.stats = None             # optional (n_games, 2) int32: levels, children scored
        if sync_free is None:
            sync_free = getattr(policy_fn, "forward_counted", None) is not None
        self.sync_free = bool(sync_free)
        if use_graph and not self.sync_free:
            raise ValueError("use_graph needs the sync-free playout (a policy with forward_counted)")
        self.use_graph, self._graph, self._graph_key = bool(use_graph), None, None
        # look-ahead blocks (of 2 K playouts) per replay of the long graph (tuning knob: DESIGN.md)
        self.graph_blocks = max(1, int(os.environ.get("IAGO_GRAPH_BLOCKS", "4")))
        self._graph_long = None
        self.n_compactions = 0
        self._live_after_compaction = 0
        # Policy look-ahead (iago_mcts_lookahead in include/iago_hip.h): leaves are queued K
        # visits before they expand and the policy net runs on the queue every K playouts, off
        # the playouts' critical path.  Default: K = 4 whenever the sync-free playout with a
        # board-fed policy net applies and n_thr leaves room for it; 0 = the net runs inside the
        # playout that expands (the reference's order of evaluation).  Same trees either way.
        # Persistent search (iago_mcts_search_persistent in include/iago_hip.h): a whole search is ONE
        # launch in which every game runs on its own clock -- game workgroups (32 games each: descent,
        # rollout, backup) and net workgroups that serve a queue of positions with the one-board walks
        # of the value and the policy net.  The policy net runs exactly where the reference runs it (at
        # the expansion), so there is no look-ahead in this mode.  Same trees.
        # (the launch keeps every game workgroup resident and needs net workgroups beside them: at most half of the
        # device's 256 CUs for the games, i.e. 4096 games per launch; larger batches take the per-playout launches)
        # (tuning knobs: pacing of the leading games -- playouts a game may be ahead of the mean while requests queue,
        # 0 = the library's default, < 0 = off; 8 / 16 / 32 games per game workgroup)
        self.pace_margin = int(os.environ.get("IAGO_PERSISTENT_PACE", "0"))
        # (games per game workgroup: 32 to 60 game workgroups measure best at every batch size -- 256 games 6.6 M leaf-evals/s
        # at 8 per workgroup against 5.1 M at 32; 512 / 640 / 768 / 896 games 11.7 / 13.1 / 14.3 / 14.5 M at 16 against 9.7 /
        # 11.2 / 12.8 / 14.0 M at 32; 1024 games 15.5 M at 32 against 14.4 M at 16: a workgroup's iteration is as long as its
        # rollout passes of 16 boards, and every game workgroup is a net workgroup less)
        self.games_per_workgroup = int(os.environ.get("IAGO_PERSISTENT_GPW", "0")) or (
            8 if n_games <= 256 else 16 if n_games <= 960 else _lib.SEARCH_GAMES_PER_WORKGROUP)
        if self.wave > 1:   # (the wave search: 32 slots per game workgroup, whole trees of them)
            self.games_per_workgroup = _lib.SEARCH_GAMES_PER_WORKGROUP
        # The launch's grid follows the device (iago_mcts_search_capacity: CUs x workgroups of the search kernel per CU,
        # all of them resident from the start); max_cus / IAGO_PERSISTENT_CUS: the CUs the launch may count on when fewer
        # are free for it -- a CU-masked stream, a device shared with another job.  The games take at most half of them
        # (4096 games per launch on a whole MI355X); larger batches take the per-playout launches.
        self.max_cus = int(max_cus if max_cus is not None else os.environ.get("IAGO_PERSISTENT_CUS", "0"))
        self.resident_workgroups = self._search_capacity()
        n_gw = -(-ns // self.games_per_workgroup)
        # Role split (iago_mcts_search_split): the game workgroups as a launch of their own, two per CU on `split` CUs
        # (a multiple of 8), the net workgroups on all the others -- two CU-masked streams, co-resident by construction.
        # Same trees.  Default ("auto"): wherever the games need more than 32 workgroups -- in the single launch every
        # game workgroup holds a CU alone, so beyond 32 of them each one is a net workgroup less; two per CU give the CUs
        # back (1536 / 2048 / 4096 games: 17.4 -> 17.9, 17.1 -> 18.3, 10.8 -> 15.1 M leaf-evals/s; 1024 games: no
        # difference, the single launch stays; LABNOTES.md, round 6).  split / IAGO_SEARCH_SPLIT: game CUs, 0 = always the single
        # launch (_split_arg refuses anything but "auto", 0 and positive multiples of 8).  Not with max_cus (the split
        # owns the device); a runtime without CU-masked streams falls back to the single launch.
        if self.wave > 1:
            want_split = 0     # (the wave search runs as the single launch)
        elif want == "auto":
            # (32-game workgroups only: the smaller workgroups of batches up to 960 games measure slower two per CU --
            # 640 / 768 / 896 games at 16 per workgroup: 14.9 / 16.3 / 16.6 M single, 13.5 / 15.1 / 16.3 M split)
            want_split = (8 * (-(-n_gw // 16)) if (n_gw > 32 and self.games_per_workgroup == _lib.SEARCH_GAMES_PER_WORKGROUP)
                          else 0)                                     # (two game workgroups per CU)
        else:
            want_split = int(want)
        self.split_cus, self._split = 0, None
        while want_split > 0 and 2 * want_split < n_gw:
            want_split += 8
        can_p = (self.resident_workgroups > 0 and 2 * n_gw <= self.resident_workgroups
                 and can_cache and getattr(value_fn, "search_args", None) is not None
                 and getattr(policy_fn, "search_args", None) is not None and getattr(policy_fn, "split3", False)
                 and rollout_weights is not None and not rollout_weights.log_form and 0.0 <= self.lmbda < 1.0
                 and ns <= _lib.SEARCH_QUEUE_ENTRIES)
        persistent = schedule(can_p)
        if persistent and not can_p:
            raise ValueError("persistent needs the split-f16 value net and the three-piece policy net (modules with "
                             "search_args), product-form rollout weights, lmbda < 1 and at most %d games (the games' "
                             "workgroups may take half of the %d workgroups this device keeps resident)"
                             % (self.resident_workgroups // 2 * self.games_per_workgroup, self.resident_workgroups))
        self.persistent = bool(persistent)
        if self.backup == "negamax" and not self.persistent:
            raise ValueError(_NEGAMAX_NEEDS)
        if self.selection == "alphazero" and not self.persistent:
            raise ValueError(_ALPHAZERO_NEEDS)
        if self.wave > 1 and not self.persistent:
            raise ValueError("wave > 1 needs the persistent search (the split-f16 value net, the three-piece policy net, "
                             "product-form rollout weights, lmbda < 1, at most %d slots)" % _lib.SEARCH_QUEUE_ENTRIES)
        if self.persistent:
            if not self.value_cache:
                raise ValueError("persistent needs the value cache")
            if (want_split > 0 and want_split % 8 == 0 and self.max_cus <= 0
                    and want_split <= self.resident_workgroups // 2):
                self._split = _search_streams(want_split)     # (None: no CU-masked streams here -> the single launch)
                self.split_cus = want_split if self._split else 0
            lookahead, async_steps, value_ahead, use_graph = 0, False, False, False
            self.use_graph = False
        can = (self.sync_free and getattr(policy_fn, "forward_counted_boards", None) is not None)
        if lookahead is None:
            k = int(os.environ.get("IAGO_LOOKAHEAD", "4"))   # (tuning knob: tools/)
            lookahead = k if (can and self.n_thr > k + 1) else 0
        # lookahead_overlap = j: the policy batch of a group of K playouts runs on a second stream
        # BESIDE the first j playouts of the next group (0: at the end of its own group, on the
        # same stream); leaves are then queued j - 1 visits earlier so that their priors are
        # stored before any of them can expand.
        if lookahead_overlap is None:
            lookahead_overlap = int(os.environ.get("IAGO_LOOKAHEAD_OVERLAP", "2"))
        self.lookahead = int(lookahead)
        j = min(int(lookahead_overlap), max(self.lookahead - 1, 0)) if self.lookahead else 0
        while j > 0 and not self.n_thr > self.lookahead + j - 1:
            j -= 1   # n_thr leaves no room to queue the leaves that much earlier
        self.lookahead_overlap = j
        margin = self.lookahead + max(self.lookahead_overlap - 1, 0)
        if z_log_rows and not self.lookahead and not self.persistent:
            raise ValueError("z_log_rows needs the look-ahead playout (rollout_hook serves the other paths)")
        if self.lookahead and not (can and self.n_thr > margin):
            raise ValueError("lookahead needs the sync-free playout, a policy net with "
                             "forward_counted_boards and n_thr > lookahead (+ overlap - 1)")
        if self.lookahead:
            K = self.lookahead
            slots = int(lookahead_slots) if lookahead_slots else max(256, capacity // 8)
            Q = n_games * K
            self._la_next_seq = torch.zeros(n_games, dtype=torch.int32, **kw)
            self._la_cache_seq = torch.full((n_games, slots), -1, dtype=torch.int32, **kw)
            self._la_cache = torch.zeros((n_games, slots, 64), dtype=torch.float32, **kw)
            self._la_error = torch.zeros(1, dtype=torch.int32, **kw)
            # the nodes of a game's last descent (the one-launch descent records them, the backup
            # updates them side by side).  A path can be much longer than the plies left: at a
            # finished position every expansion adds one more pass child (MCTS.py:112-114), so the
            # buffer covers the descent's own bound of 512 levels
            self.PATH_STRIDE = 520
            self.fused_descent = os.environ.get("IAGO_FUSED_DESCENT", "1") != "0"
            use_path = self.fused_descent and os.environ.get("IAGO_BACKUP_PATH", "1") != "0"
            self._la_path = torch.zeros((n_games, self.PATH_STRIDE), dtype=torch.int32, **kw) if use_path else None
            self._la_path_len = torch.zeros(n_games, dtype=torch.int32, **kw) if use_path else None
            # two queues: the playouts of a group fill one while the other one's batch is in flight
            self._la_queues, self._la = [], []
            # diagnostic record of the parity tests: the z every playout of a game backed up, in
            # playout order (iago_mcts_lookahead.z_log); works in graph mode, unlike rollout_hook
            self.z_log = torch.zeros((z_log_rows, n_games), dtype=torch.int8, **kw) if z_log_rows else None
            self.z_log_n = torch.zeros(n_games, dtype=torch.int32, **kw) if z_log_rows else None
            for _ in range(2):
                q = dict(count=torch.zeros(1, dtype=torch.int32, **kw), own=torch.zeros(Q, dtype=torch.int64, **kw),
                         opp=torch.zeros(Q, dtype=torch.int64, **kw), game=torch.zeros(Q, dtype=torch.int32, **kw),
                         seq=torch.zeros(Q, dtype=torch.int32, **kw))
                a = _lib.MctsLookahead()
                a.trigger, a.slots, a.q_capacity = self.n_thr - margin, slots, Q
                a.next_seq, a.cache_seq = self._la_next_seq.data_ptr(), self._la_cache_seq.data_ptr()
                a.cache, a.q_count = self._la_cache.data_ptr(), q["count"].data_ptr()
                a.q_own, a.q_opp = q["own"].data_ptr(), q["opp"].data_ptr()
                a.q_game, a.q_seq = q["game"].data_ptr(), q["seq"].data_ptr()
                a.error = self._la_error.data_ptr()
                # the backup clears the fresh-leaf count that the next descent appends to
                a.clear_word = self._fresh_count.data_ptr() if self.value_cache else None
                if self._la_path is not None:
                    a.path, a.path_len = self._la_path.data_ptr(), self._la_path_len.data_ptr()
                    a.path_stride = self.PATH_STRIDE
                if self.z_log is not None:
                    a.z_log, a.z_log_n, a.z_log_rows = self.z_log.data_ptr(), self.z_log_n.data_ptr(), z_log_rows
                self._la_queues.append(q)
                self._la.append(a)
            self._la_cur = 0   # the queue the playouts fill
            prio = int(os.environ.get("IAGO_SIDE_PRIORITY", "0"))
            self._la_side = torch.cuda.Stream(device=device, priority=prio) if self.lookahead_overlap else None
            # Value look-ahead (iago_mcts_value_ahead in include/iago_hip.h): the descent queues every
            # node it expands; once per group of K playouts the children that have no value yet go
            # through the value net as ONE batch on the side stream and the results land in the
            # children's records, so that their first visits find a stored value instead of walking
            # the net on the playouts' critical path.  Same trees (a child visited before its value
            # has landed is evaluated in place as before).  Default OFF -- measured slower (round 4,
            # LABNOTES.md): in lockstep ONE game without a stored value still puts a 70 us one-board
            # walk on every playout's critical path (1024 games x 16 % fresh leaves x 53 % misses = ~85
            # per playout), and with game-asynchronous steps the extra evaluations (children that are
            # never visited, or visited before their value lands: +50 % rows) make the side stream the
            # bound.  value_ahead=True / IAGO_VALUE_AHEAD=1 selects it.
            can_va = bool(self.value_cache and self.fused_descent and self._la_side is not None
                          and getattr(value_fn, "forward_boards_batch", None) is not None)
            if value_ahead is None:
                value_ahead = can_va and os.environ.get("IAGO_VALUE_AHEAD", "0") == "1"
            if value_ahead and not can_va:
                raise ValueError("value_ahead needs the value cache, the one-launch descent, lookahead_overlap > 0 "
                                 "and a value net with forward_boards_batch")
            self.value_ahead = bool(value_ahead)
            if self.value_ahead:
                self.va_boards = int(os.environ.get("IAGO_VALUE_AHEAD_BOARDS", "2"))      # boards per workgroup
                self.va_grid = int(os.environ.get("IAGO_VALUE_AHEAD_GRID", "176"))        # workgroup cap of a batch
                xcap, rcap = n_games * K, max(4096, 8 * n_games * K)
                self._va_total = torch.zeros(1, dtype=torch.int64, **kw)   # rows the batches have evaluated
                self._va_row_count = torch.zeros(1, dtype=torch.int32, **kw)
                self._va_rows = dict(own=torch.zeros(rcap, dtype=torch.int64, **kw),
                                     opp=torch.zeros(rcap, dtype=torch.int64, **kw),
                                     node=torch.zeros(rcap, dtype=torch.int64, **kw),
                                     v=torch.zeros(rcap, dtype=torch.float32, **kw))
                self._va_x, self._va = [], []
                for a in self._la:
                    x = dict(count=torch.zeros(1, dtype=torch.int32, **kw), game=torch.zeros(xcap, dtype=torch.int32, **kw),
                             node=torch.zeros(xcap, dtype=torch.int32, **kw), own=torch.zeros(xcap, dtype=torch.int64, **kw),
                             opp=torch.zeros(xcap, dtype=torch.int64, **kw))
                    v = _lib.MctsValueAhead()
                    v.x_capacity, v.row_capacity = xcap, rcap
                    v.x_count, v.x_game, v.x_node = x["count"].data_ptr(), x["game"].data_ptr(), x["node"].data_ptr()
                    v.x_own, v.x_opp = x["own"].data_ptr(), x["opp"].data_ptr()
                    v.row_count = self._va_row_count.data_ptr()
                    v.row_own, v.row_opp = self._va_rows["own"].data_ptr(), self._va_rows["opp"].data_ptr()
                    v.row_node, v.row_v = self._va_rows["node"].data_ptr(), self._va_rows["v"].data_ptr()
                    v.total = self._va_total.data_ptr()
                    a.value_ahead = C.addressof(v)
                    self._va_x.append(x)
                    self._va.append(v)
                self._ev_priors = torch.cuda.Event()
                self._ev_rows = torch.cuda.Event()

            # games whose cached priors were computed by policy weights that have changed since (search() refreshes
            # them when the game next searches: its roots are known then)
            self._la_stale = torch.zeros(n_games, dtype=torch.bool, **kw)
            self._la_stale_any = False

            def reset_lookahead(mask):
                if mask is None:
                    self._la_next_seq.zero_()
                    self._la_cache_seq.fill_(-1)
                    self._la_stale.zero_()
                else:
                    m = mask.bool()
                    self._la_next_seq[m] = 0
                    self._la_cache_seq[m] = -1
                    self._la_stale[m] = False
            self.tree.reset_hooks = [reset_lookahead]
        self.value_ahead = bool(getattr(self, "value_ahead", False))
        if self.persistent:
            if net_workgroups is None:
                net_workgroups = int(os.environ.get("IAGO_PERSISTENT_NET", "0")) or max(32, 8 * n_games)
            # (an upper bound: the launch itself takes no more than fit beside the game workgroups)
            self.net_workgroups = max(1, min(int(net_workgroups), self.resident_workgroups - n_gw))
            if self.split_cus:   # (one net workgroup on every CU that is not the games', at most 7/8 of the device's CUs:
                # the library's cap -- beyond it the net launch's last workgroups were seen to stall, LABNOTES.md round 6)
                self.net_workgroups = max(1, min(int(net_workgroups), self.resident_workgroups
                                                 - max(self.split_cus, self.resident_workgroups // 8)))
            grid = n_gw + self.net_workgroups
            self.PATH_STRIDE = 520 if path_stride is None else int(path_stride)
            i64 = torch.int64
            self._ps = dict(
                path=torch.zeros((ns, self.PATH_STRIDE), dtype=torch.int32, **kw),
                done=torch.zeros(ns, dtype=torch.int32, **kw), roll=torch.zeros(ns, dtype=torch.uint8, **kw),
                q_slots=torch.zeros(2 * _lib.SEARCH_QUEUE_ENTRIES * 8, dtype=i64, **kw), ctl=torch.zeros(16, dtype=torch.int32, **kw),
                rep_v=torch.zeros(ns, dtype=i64, **kw), rep_p=torch.zeros(ns * 64, dtype=i64, **kw),
                totals=torch.zeros(17, dtype=i64, **kw), wg_own=torch.zeros(4 * grid, dtype=i64, **kw),
                wg_opp=torch.zeros(4 * grid, dtype=i64, **kw), wg_v=torch.zeros(4 * grid, dtype=torch.float32, **kw),
                wg_probs=torch.zeros((4 * grid, 64), dtype=torch.float32, **kw))
            # position table of the value net (iago_mcts_search_args.vtable): 2^20 entries of 32 bytes, shared by the
            # games and kept across launches; zeroed when the value net's weights change
            slots = int(os.environ.get("IAGO_PERSISTENT_TABLE", str(1 << 20)))
            self._vtable = torch.zeros(4 * slots, dtype=i64, **kw) if slots > 0 else None
            self.z_log = torch.zeros((z_log_rows, n_games), dtype=torch.int8, **kw) if z_log_rows else None
            self.z_log_n = torch.zeros(n_games, dtype=torch.int32, **kw) if z_log_rows else None
            self.time_limit_ms = int(os.environ.get("IAGO_PERSISTENT_LIMIT_MS", "4000"))
            # (the wave search's game-workgroup time, 100 MHz ticks: descents, rollouts, backups, waits; tools/time_wave.py)
            self.wave_timing = torch.zeros(4, dtype=i64, **kw)
            self._wave_active = None
        self.tree.reset_hooks = list(getattr(self.tree, "reset_hooks", ())) + [
            lambda mask: setattr(self, "_live_after_compaction", 0)]
        # Game-asynchronous steps (iago_mcts_async in include/iago_hip.h): a game whose leaf has a
        # stored value completes its playout in the step; a game whose leaf is fresh waits `parts`
        # steps while the value net walks its board piece by piece beside the other games' steps.
        # Same trees (tests/test_mcts_production_gpu.py runs both schedules against the oracle).
        # Default OFF: measured slower than lockstep playouts as long as every search ends in
        # lockstep -- a 100-playout search needs ~200 steps of ~105 us because the game with the most
        # fresh leaves sets the step count (LABNOTES.md, round 3); async_steps=True / IAGO_ASYNC=1
        # selects it.
        can_async = bool(self.lookahead and self.value_cache and getattr(self, "fused_descent", False)
                         and getattr(self, "_la_path", None) is not None and self.fused_leaf_eval
                         and 0.0 < self.lmbda < 1.0 and rollout_weights is not None and not rollout_weights.log_form
                         and getattr(value_fn, "forward_boards_async", None) is not None)
        if async_steps is None:
            async_steps = can_async and os.environ.get("IAGO_ASYNC", "0") == "1"
        if async_steps and not can_async:
            raise ValueError("async_steps needs the look-ahead playout with the value cache, the one-launch descent, "
                             "the path backup, the fused leaf evaluation (0 < lmbda < 1, product-form rollout "
                             "weights) and a value net with forward_boards_async")
        self.async_steps = bool(async_steps)
        self.n_steps = 0              # game-asynchronous steps run so far
        if self.async_steps:
            parts = int(async_parts if async_parts is not None else os.environ.get("IAGO_ASYNC_PARTS", "3"))
            if not 2 <= parts <= 4:
                raise ValueError("async_parts must be 2, 3 or 4")
            self.async_parts = parts
            self._a_wait = torch.zeros(n_games, dtype=torch.int32, **kw)
            self._a_done = torch.zeros(n_games, dtype=torch.int32, **kw)
            self._a_roll = torch.zeros(n_games, dtype=torch.uint8, **kw)
            self._a_fq_index = torch.zeros((parts, n_games), dtype=torch.int64, **kw)
            self._a_fq_count = torch.zeros(parts, dtype=torch.int32, **kw)
            self._a_step = torch.zeros(1, dtype=torch.int32, **kw)
            self._a_nsims = torch.zeros(1, dtype=torch.int32, **kw)
            self._a_scratch = torch.empty((parts, n_games, _lib.VALUE_IMAGE_BYTES), dtype=torch.uint8, **kw)
            y = _lib.MctsAsync()
            y.parts = parts
            y.wait, y.done, y.roll = self._a_wait.data_ptr(), self._a_done.data_ptr(), self._a_roll.data_ptr()
            y.fq_index, y.fq_count = self._a_fq_index.data_ptr(), self._a_fq_count.data_ptr()
            y.step, y.n_sims, y.scratch = self._a_step.data_ptr(), self._a_nsims.data_ptr(), self._a_scratch.data_ptr()
            self._async = y
            # the look-ahead state of the asynchronous steps: the lockstep one + the pointer
            self._la_async = []
            for a in self._la:
                b = _lib.MctsLookahead.from_buffer_copy(a)
                b.async_ = C.addressof(y)
                self._la_async.append(b)
            self._async_hint = {}     # n_sims -> steps the last such search needed
        self._g_own = torch.zeros(n_games, dtype=torch.int64, **kw)
        self._g_opp = torch.zeros(n_games, dtype=torch.int64, **kw)
        self._g_active = torch.zeros(n_games, dtype=torch.uint8, **kw)
        self._sim_dev = torch.zeros(1, dtype=torch.int32, **kw)  # Philox stream id on the device
        self.sim_counter = 0          # Philox stream id: one per simulation
        self.n_leaf_evals = 0
        self._n_policy_host = 0
        self.rollout_hook = None
        self._rollout_out = ops.RolloutResult()
        self._rollout_out.z = self.z

    def _search_capacity(self):
        """Workgroups of the persistent search this device keeps resident (0: the kernel cannot run here)."""
        cus, per = C.c_int32(0), C.c_int32(0)
        if _lib.lib().iago_mcts_search_capacity(C.byref(cus), C.byref(per)) != 0:
            return 0
        n = cus.value if self.max_cus <= 0 else min(self.max_cus, cus.value)
        return n * per.value

    # policy evaluations so far: counted on the host (host-counted playouts) and on the
    # device (sync-free playouts; reading it is a host sync)
    @property
    def n_policy_evals(self):
        if self.persistent:   # (+ the per-playout launches a rollout hook sends the searches through)
            return int(self._ps["totals"][1].item()) + self._n_policy_host + int(self._pend_total.item())
        return self._n_policy_host + int(self._pend_total.item())

    @property
    def n_value_evals(self):
        """Value-net evaluations executed so far: with the value cache the first visits of leaves that
        had no stored value (n_value_inline) + the rows of the value look-ahead's batches
        (n_value_ahead)."""
        return self.n_value_inline + self.n_value_ahead if self.value_cache else self.n_leaf_evals

    @property
    def n_value_inline(self):
        """Evaluations on the playouts' critical path (a leaf visited before it had a value)."""
        if self.persistent:
            return int(self._ps["totals"][0].item()) + int(self._value_total.item())
        return int(self._value_total.item()) if self.value_cache else self.n_leaf_evals

    @property
    def n_value_ahead(self):
        """Evaluations off the critical path: rows the value look-ahead's batches have evaluated (hits, duplicates and
        never-visited); with the persistent search the positions idle net workgroups walked for the position table
        ahead of their first visit (the children of expanding nodes)."""
        if self.persistent:
            return int(self._ps["totals"][11].item())
        return int(self._va_total.item()) if self.value_ahead else 0

    @n_policy_evals.setter
    def n_policy_evals(self, value):
        if value != 0:
            raise ValueError("n_policy_evals can only be reset to 0")
        self._n_policy_host = 0
        self._pend_total.zero_()
        if self.persistent:
            self._ps["totals"][1].zero_()

    def _bucket(self, n):
        """Smallest power-of-two batch >= n (min 16), capped at the pool size."""
        b = 16
        while b < n:
            b *= 2
        return min(b, self._policy_in.shape[0])

    def warmup(self):
        """Run the nets once per batch shape the search will use."""
        with torch.no_grad():
            if self.policy_fn is not None and self.sync_free:
                self._policy_counted(self._policy_in[:self.n_games], self._pend_count)
            elif self.policy_fn is not None:
                b = 16
                while True:
                    nb = min(b, self._policy_in.shape[0])
                    self.policy_fn(self._policy_in[:nb])
                    if nb == self._policy_in.shape[0]:
                        break
                    b *= 2
            if self.value_fn is not None and self.lmbda < 1.0:
                self.value_fn(self.planes)
        torch.cuda.synchronize()

    # -- one simulation = MCTS.playout for every active game (MCTS.py:105-133)
    def _select(self, own, opp, active, from_root):
        L = _lib.lib()
        check(L.iago_mcts_select(self.tree.ref(), _p(own), _p(opp), _p(active), self.c_puct,
                                 self.n_thr, 1 if from_root else 0, _p(self.cur_node),
                                 _p(self.cur_own), _p(self.cur_opp), _p(self.needs_expand),
                                 _p(self.legal), _p(self.stats) if self.stats is not None else None,
                                 _stream()), "iago_mcts_select")

    def _find_pending(self, active):
        check(_lib.lib().iago_mcts_pending(_p(self.needs_expand), _p(active), self.n_games,
                                           _p(self._pending), _p(self._pend_idx), _p(self._pend_games),
                                           _p(self._pend_count),
                                           _p(self._pend_total) if self.sync_free else None,
                                           _stream()), "iago_mcts_pending")

    def _expand_pending(self, own, opp, active):
        """Expansion branch of MCTS.playout (MCTS.py:109-121) for the games whose
        cursor sits on a leaf with n_visits >= n_thr, host-counted: one host sync."""
        L = _lib.lib()
        self._find_pending(active)
        n_exp = int(self._pend_count.item())  # the one host sync of a playout
        if n_exp == 0:
            return
        pending, idx, games = self._pending, self._pend_idx[:n_exp], self._pend_games[:n_exp]
        # MIOpen picks (and on first sight searches for) a kernel per input
        # shape: run the policy net on a few fixed bucket sizes only
        nb = self._bucket(n_exp)
        sub_planes = self._policy_in[:nb]
        ops.encode_planes_indexed(self.cur_own, self.cur_opp, idx, sub_planes)
        with torch.no_grad():
            probs = self.policy_fn(sub_planes).to(torch.float32).contiguous()
        self._n_policy_host += n_exp
        check(L.iago_mcts_expand(self.tree.ref(), _p(games), games.numel(), _p(self.cur_node),
                                 _p(self.legal), _p(probs), None, _stream()), "iago_mcts_expand")
        self._select(own, opp, pending, False)  # MCTS.py:121: recurse into the same node

    def _policy_counted(self, planes, n_dev):
        """(len(planes), 64) float32 probabilities, valid in the first *n_dev rows."""
        fc = getattr(self.policy_fn, "forward_counted", None)
        with torch.no_grad():
            if fc is not None:
                return fc(planes, n_dev)
            return self.policy_fn(planes).to(torch.float32).contiguous()

    def _expand_pending_counted(self, own, opp, active):
        """The same branch with the count left on the device: every launch is enqueued
        unconditionally and sized for n_games; items past *count exit at once."""
        L = _lib.lib()
        self._find_pending(active)
        n = self.n_games
        fb = getattr(self.policy_fn, "forward_counted_boards", None)
        if fb is not None:  # plane encoding fused into the net's first layer
            probs = fb(self.cur_own, self.cur_opp, self._pend_idx, n, self._pend_count)
        else:
            planes = self._policy_in[:n]
            ops.encode_planes_indexed(self.cur_own, self.cur_opp, self._pend_idx, planes,
                                      n_dev=self._pend_count)
            probs = self._policy_counted(planes, self._pend_count)
        check(L.iago_mcts_expand(self.tree.ref(), _p(self._pend_games), n, _p(self.cur_node),
                                 _p(self.legal), _p(probs), _p(self._pend_count), _stream()),
              "iago_mcts_expand")
        self._select(own, opp, self._pending, False)  # MCTS.py:121: recurse into the same node

    def _evaluate_and_backup(self, active, stream_id=0, stream_id_dev=None, counter=None, fresh_listed=False):
        """Leaf evaluation (MCTS.py:123-127) and Node.update_recursive."""
        L = _lib.lib()
        rolled = False  # the rollout has run inside the value net's launch
        if self.lmbda < 1.0 and self.value_cache:
            # the value net on the leaves without a stored value only (device-side list + count)
            if not fresh_listed:
                check(L.iago_mcts_fresh_leaves(self.tree.ref(), _p(active), _p(self.cur_node), _p(self._fresh_idx),
                                               _p(self._fresh_count), _p(self._value_total), _stream()),
                      "iago_mcts_fresh_leaves")
            # ... and, in the same launch, the rollouts of all leaves (two kinds of workgroups)
            both = (self.fused_leaf_eval and self.lmbda > 0.0 and self.rollout_hook is None
                    and self.rollout_weights is not None and not self.rollout_weights.log_form)
            ro = None
            if both:
                ro = ops.rollout_prepare(self.cur_own, self.cur_opp, self.rollout_weights, seed=self.seed,
                                         id_base=self.game_id_base, stream_id=stream_id,
                                         stream_id_dev=stream_id_dev, out=self._rollout_out)
            with torch.no_grad():
                self.value_fn.forward_boards_counted(self.cur_own, self.cur_opp, self._fresh_idx,
                                                     self._fresh_count, self.v, rollout=ro)
            rolled = both
        elif self.lmbda < 1.0:
            v = None
            fb = getattr(self.value_fn, "forward_boards", None)
            with torch.no_grad():
                if fb is not None:
                    v = fb(self.cur_own, self.cur_opp)  # plane encoding fused into the first layer
                if v is None:
                    ops.encode_planes(self.cur_own, self.cur_opp, out=self.planes)
                    v = self.value_fn(self.planes)
            self.v = v.to(torch.float32).contiguous()
        if self.lmbda > 0.0 and not rolled:
            ops.rollout(self.cur_own, self.cur_opp, self.rollout_weights, seed=self.seed,
                        id_base=self.game_id_base, stream_id=stream_id,
                        stream_id_dev=stream_id_dev, out=self._rollout_out)
            if self.rollout_hook is not None:
                self.rollout_hook(self)
        if self.lookahead:
            check(L.iago_mcts_mix_backup_lookahead(
                self.tree.ref(), _p(active), _p(self.cur_node), _p(self.cur_own), _p(self.cur_opp),
                _p(self.v) if self.lmbda < 1.0 else None, _p(self.z) if self.lmbda > 0.0 else None,
                self.lmbda, _p(self.leaf_value), _p(counter) if counter is not None else None,
                C.byref(self._la[self._la_cur]), _stream()), "iago_mcts_mix_backup_lookahead")
            return
        check(L.iago_mcts_mix_backup(self.tree.ref(), _p(active), _p(self.cur_node),
                                     _p(self.v) if self.lmbda < 1.0 else None,
                                     _p(self.z) if self.lmbda > 0.0 else None, self.lmbda,
                                     _p(self.leaf_value), _p(counter) if counter is not None else None,
                                     _stream()), "iago_mcts_mix_backup")

    def _playout_lookahead(self, own, opp, active, stream_id=0, stream_id_dev=None, counter=None):
        """One MCTS.playout for every active game with the priors of the expanding leaves taken
        from the look-ahead cache: select, expand, continue the descent, evaluate, back up (and
        queue the leaves that are K visits from expanding)."""
        L = _lib.lib()
        if self.fused_descent:
            # select, expand from the cache, continue, list the leaves without a value: one launch
            check(L.iago_mcts_descend(self.tree.ref(), _p(own), _p(opp), _p(active), self.c_puct, self.n_thr,
                                      _p(self.cur_node), _p(self.cur_own), _p(self.cur_opp), _p(self.legal),
                                      _p(self.stats) if self.stats is not None else None,
                                      C.byref(self._la[self._la_cur]),   # (the group's queue of expanded nodes)
                                      _p(self._fresh_idx) if self.value_cache else None,
                                      _p(self._fresh_count) if self.value_cache else None,
                                      _p(self._value_total) if self.value_cache else None, _stream()),
                  "iago_mcts_descend")
            self._evaluate_and_backup(active, stream_id=stream_id, stream_id_dev=stream_id_dev, counter=counter,
                                      fresh_listed=self.value_cache)
            return
        self._select(own, opp, active, True)
        check(L.iago_mcts_expand_cached(self.tree.ref(), _p(active), _p(self.needs_expand), _p(self.cur_node),
                                        _p(self.legal), C.byref(self._la[0]), _p(self._pending), _stream()),
              "iago_mcts_expand_cached")
        self._select(own, opp, self._pending, False)  # MCTS.py:121: recurse into the same node
        self._evaluate_and_backup(active, stream_id=stream_id, stream_id_dev=stream_id_dev, counter=counter)

    def _step_async(self, own, opp, active):
        """One game-asynchronous step for every game of `active`: descent of the games that are not
        waiting, leaf evaluation (rollouts of those games + one piece of the value net per queue of
        fresh leaves), backup of the games whose playout completes in this step."""
        L = _lib.lib()
        check(L.iago_mcts_descend(self.tree.ref(), _p(own), _p(opp), _p(active), self.c_puct, self.n_thr,
                                  _p(self.cur_node), _p(self.cur_own), _p(self.cur_opp), _p(self.legal),
                                  _p(self.stats) if self.stats is not None else None,
                                  C.byref(self._la_async[self._la_cur]),
                                  None, None, _p(self._value_total), _stream()), "iago_mcts_descend")
        ro = self.__dict__.get("_async_rollout")
        if ro is None or ro._keep[2] is not self.rollout_weights:
            # (marshalled once: the Philox stream of game g's playout is stream base + done[g], the
            # base in the device word the search sets)
            ro = self._async_rollout = ops.rollout_prepare(
                self.cur_own, self.cur_opp, self.rollout_weights, seed=self.seed, id_base=self.game_id_base,
                stream_id=0, stream_id_dev=self._sim_dev, out=self._rollout_out)
        with torch.no_grad():
            self.value_fn.forward_boards_async(self.cur_own, self.cur_opp, self.v, ro, C.byref(self._async))
        check(L.iago_mcts_mix_backup_lookahead(
            self.tree.ref(), _p(active), _p(self.cur_node), _p(self.cur_own), _p(self.cur_opp), _p(self.v), _p(self.z),
            self.lmbda, _p(self.leaf_value), None, C.byref(self._la_async[self._la_cur]), _stream()),
            "iago_mcts_mix_backup_lookahead")

    def _flush_lookahead(self, which=0):
        """The policy net on the leaves of queue `which` (one batch), its outputs into the prior
        cache; the queue is empty afterwards."""
        q = self._la_queues[which]
        n = q["own"].numel()
        probs = self.policy_fn.forward_counted_boards(q["own"], q["opp"], None, n, q["count"])
        check(_lib.lib().iago_mcts_store_priors(C.byref(self._la[which]), _p(probs), _p(self._pend_total),
                                                _stream()), "iago_mcts_store_priors")
        q["count"].zero_()

    def _refresh_priors(self, own, opp, active):
        """The policy net's weights changed since the look-ahead cached the priors of leaves that have not expanded
        yet: those priors again, from the current weights (the reference evaluates the net when the leaf expands,
        MCTS.py:109-121), for the games of `active` whose priors are stale.  Each leaf's position is rebuilt from its
        game's root by the moves of its path -- own / opp of an active game ARE its root's position; a game outside
        `active` stays marked until it searches -- and a leaf no longer under its game's root (left behind by
        update_with_move) is skipped: it never expands."""
        games = self._la_stale & (active != 0)
        self._la_stale &= ~games
        self._la_stale_any = bool(self._la_stale.any().item())
        t, S = self.tree, self._la[0].slots
        dev, cap = t.nodes.device, t.capacity
        fc = t.first_child.reshape(t.n_games, cap)
        seq = (-2 - fc).clamp(min=0)
        cached = self._la_cache_seq.gather(1, (seq % S).to(torch.int64)) == seq
        live = torch.arange(cap, device=dev).reshape(1, cap) < t.n_nodes.reshape(-1, 1)
        g, node = torch.nonzero(live & (fc <= -2) & cached & games.reshape(-1, 1), as_tuple=True)
        if g.numel() == 0:
            return
        base, root = g * cap, t.root[g].to(torch.int64)
        cur, on = node.clone(), node != root
        acts, steps = [], []
        while bool(on.any().item()):   # (leaf to root, one level per pass)
            acts.append(torch.where(on, t.action[base + cur].to(torch.int8), torch.full_like(node, -1, dtype=torch.int8)))
            steps.append(on.clone())
            up = t.parent[base + cur].to(torch.int64)
            cur = torch.where(on & (up >= 0), up, cur)
            on = on & (up >= 0) & (cur != root)
        keep = cur == root
        o, p = own[g].clone(), opp[g].clone()
        for a, s in zip(reversed(acts), reversed(steps)):   # (root to leaf: the mover's stone, then the other side moves)
            ops.apply_moves(o, p, a)
            o, p = torch.where(s, p, o), torch.where(s, o, p)
        g, slot, o, p = g[keep], (seq[g, node] % S)[keep], o[keep], p[keep]
        n = int(g.numel())
        if n == 0:
            return
        with torch.no_grad():
            probs = self.policy_fn.forward_counted_boards(o.contiguous(), p.contiguous(), None, n,
                                                          torch.full((1,), n, dtype=torch.int32, device=dev))
        self._la_cache[g, slot] = probs[:n]

    def _flush_value_ahead(self, which, rows_event=None):
        """The value look-ahead's batch for the nodes queue `which` holds: one row per child without a
        value, the value net on the rows, the results into the children's records.  rows_event: recorded
        once the queue has been consumed (the next group may then append to it)."""
        L = _lib.lib()
        va, rows = self._va[which], self._va_rows
        self._va_row_count.zero_()
        check(L.iago_mcts_value_ahead_rows(self.tree.ref(), C.byref(va), _stream()), "iago_mcts_value_ahead_rows")
        self._va_x[which]["count"].zero_()
        if rows_event is not None:
            rows_event.record()
        with torch.no_grad():
            self.value_fn.forward_boards_batch(rows["own"], rows["opp"], self._va_row_count, rows["v"],
                                               self.va_boards, self.va_grid)
        check(L.iago_mcts_value_ahead_store(self.tree.ref(), C.byref(va), _stream()), "iago_mcts_value_ahead_store")

    def _lookahead_block(self, own, opp, active, stream_ids, async_=False, last=True):
        """Two groups of K playouts.  On entry queue 1 may hold the leaves of the previous block's
        second group and queue 0 is empty; on exit the same.  With lookahead_overlap = j > 0 the
        batch of the previous group runs on the side stream beside the first j playouts of a group
        (its leaves were queued early enough for that); with 0 every group ends with its own
        batch on the one stream.  stream_ids: None (the device word, graph capture / replay) or an
        iterator of 2 K Philox stream ids."""
        K, j = self.lookahead, self.lookahead_overlap
        main = torch.cuda.current_stream()
        va = self.value_ahead
        for grp in (0, 1):
            self._la_cur = grp
            if j:
                self._la_side.wait_stream(main)
                with torch.cuda.stream(self._la_side):
                    self._flush_lookahead(1 - grp)
                    if va:
                        # the value batch of the previous group's expansions goes on beside this whole
                        # group; the playouts only wait for the priors (playout j) and, before the next
                        # group appends to the queue, for the rows kernel that consumes it
                        self._ev_priors.record()
                        self._flush_value_ahead(1 - grp, self._ev_rows)
            for i in range(K):
                if j and i == j:
                    if va:
                        main.wait_event(self._ev_priors)
                    else:
                        main.wait_stream(self._la_side)
                if async_:
                    self._step_async(own, opp, active)
                elif stream_ids is None:
                    self._playout_lookahead(own, opp, active, stream_id=0, stream_id_dev=self._sim_dev,
                                            counter=self._sim_dev)
                else:
                    self._playout_lookahead(own, opp, active, stream_id=next(stream_ids))
            if not j:
                self._flush_lookahead(grp)
            if va:
                main.wait_event(self._ev_rows)
        if va and last:
            main.wait_stream(self._la_side)   # (a captured graph ends with every stream joined)
        self._la_cur = 0

    def _lookahead_tail(self, own, opp, active, n, stream_ids):
        """The rest of a search after its whole blocks: queue 1's batch, then n < 2 K playouts with
        a batch after every K of them and at the end (one stream); both queues end empty."""
        if self.lookahead_overlap:
            self._flush_lookahead(1)
        if self.value_ahead:
            self._flush_value_ahead(1)
        self._la_cur = 0
        for i in range(n):
            if stream_ids is None:
                self._playout_lookahead(own, opp, active, stream_id=0, stream_id_dev=self._sim_dev,
                                        counter=self._sim_dev)
            else:
                self._playout_lookahead(own, opp, active, stream_id=next(stream_ids))
            if (i + 1) % self.lookahead == 0 or i + 1 == n:
                self._flush_lookahead(0)
                if self.value_ahead:
                    self._flush_value_ahead(0)

    def simulate(self, own, opp, active, n_active=None):
        """One MCTS.playout for every active game (eager launches)."""
        if self.lookahead:
            self._la_cur = 0
            self._playout_lookahead(own, opp, active, stream_id=self.sim_counter)
            self._flush_lookahead(0)  # a lone playout flushes at once: the queues are empty between calls
            if self.value_ahead:
                self._flush_value_ahead(0)
            self.sim_counter = (self.sim_counter + 1) & 0xFFFFFFFF
            if n_active is not None:
                self.n_leaf_evals += n_active
            return
        self._select(own, opp, active, True)
        if self.sync_free:
            self._expand_pending_counted(own, opp, active)
        else:
            self._expand_pending(own, opp, active)
        self._evaluate_and_backup(active, stream_id=self.sim_counter)
        self.sim_counter = (self.sim_counter + 1) & 0xFFFFFFFF
        if n_active is not None:
            self.n_leaf_evals += n_active

    # -- hipGraph mode: the whole sync-free playout is captured once and replayed with a
    # single launch per playout; the rollout's Philox stream id is a device word the graph
    # itself increments.
    def _graph_state(self):
        """What the captured graph baked in: device pointers and versions of every weight
        (and of the layouts cached from them), the rollout table, the scalar arguments."""
        key = [self.lmbda, self.c_puct, self.n_thr, self.lookahead, self.lookahead_overlap, self.value_cache,
               self.async_steps, self.value_ahead, self.persistent,
               getattr(self, "fused_descent", False), self.fused_leaf_eval,
               self.stats.data_ptr() if self.stats is not None else 0,
               self.rollout_weights.table.data_ptr() if self.rollout_weights is not None else 0]
        for fn in (self.policy_fn, self.value_fn):
            params = getattr(fn, "parameters", None)
            if params is not None:
                key.extend((q.data_ptr(), q._version) for q in params())
                key.append(bool(getattr(fn, "training", False)))
                key.append(bool(getattr(fn, "split_f16", False)))
                key.append(bool(getattr(fn, "fused", False)))
                key.append((getattr(fn, "split3", None), getattr(fn, "split3_parts", None)))
            else:
                key.append(id(fn))
        return tuple(key)

    def close(self):
        """Drop the captured graphs (and with them their private memory pools) now.  An engine
        holds reference cycles (the trees' reset hooks), so without this its graphs live until the
        cyclic garbage collector runs -- which must not happen while ANOTHER engine captures:
        destroying a graph is not permitted while a stream of the process is capturing."""
        self._graph = self._graph_long = self._graph_key = None
        self._scratch_refs = None

    def _capture(self):
        """Record the playout launches into hipGraphs.  The cyclic garbage collector is held
        off for the duration: a collected torch.cuda.CUDAGraph of some other, unreferenced engine
        would be destroyed inside the capture, which HIP refuses (hipErrorStreamCaptureUnsupported)."""
        import gc
        self._graph = self._graph_long = None
        self._scratch_refs = None
        gc.collect()
        # (this engine's old graphs are gone and with them its hold on the scratch buffers of the
        # policy's multi-launch forward: the module drops its own references -- 205 MB per calling
        # stream that a re-capture-per-update loop would otherwise pile up -- and the warm-up below
        # allocates what the new capture needs.  Another engine that shares the module keeps the
        # buffers ITS graphs address alive through its own _scratch_refs)
        rel = getattr(self.policy_fn, "release_scratch", None)
        if rel is not None:
            rel()
        was_enabled = gc.isenabled()
        gc.disable()
        try:
            self._capture_graphs()
            pool = getattr(self.policy_fn, "__dict__", {}).get("_split3_scratch_pool", {})
            self._scratch_refs = [b for k, b in pool.items() if k != "retired"] + list(pool.get("retired", ()))
        finally:
            if was_enabled:
                gc.enable()

    def _capture_graphs(self):
        if self.rollout_hook is not None:
            raise ValueError("rollout_hook is not available in graph mode")
        # one eager evaluation of both nets first: lazy one-time setup (kernel attributes,
        # MIOpen's choice for this shape, weight layouts cached per weight version) must not
        # happen under capture.  Neither touches the trees.
        if self.lmbda < 1.0 and self.value_cache:
            # (through the very entry point the capture records -- iago_value_rollout when the leaf
            # evaluation is fused -- with an empty fresh list: the value rows do nothing, the
            # rollouts write self.z, which every playout overwrites before it is read)
            self._fresh_count.zero_()
            both = (self.fused_leaf_eval and self.lmbda > 0.0 and self.rollout_weights is not None
                    and not self.rollout_weights.log_form)
            ro = ops.rollout_prepare(self.cur_own, self.cur_opp, self.rollout_weights, seed=self.seed,
                                     id_base=self.game_id_base, stream_id=0, stream_id_dev=self._sim_dev,
                                     out=self._rollout_out) if both else None
            with torch.no_grad():
                self.value_fn.forward_boards_counted(self.cur_own, self.cur_opp, self._fresh_idx,
                                                     self._fresh_count, self.v, rollout=ro)
        elif self.lmbda < 1.0:
            ops.encode_planes(self.cur_own, self.cur_opp, out=self.planes)
            with torch.no_grad():
                fb = getattr(self.value_fn, "forward_boards", None)
                if fb is None or fb(self.cur_own, self.cur_opp) is None:
                    self.value_fn(self.planes)
        if self.policy_fn is not None:
            # the entry point _expand_pending_counted / _flush_lookahead take: the board-fed forward
            # (three-piece kernel: weight split, argument template, scratch buffer, kernel
            # attributes) when the policy has one, the planes-fed float32 kernels otherwise
            self._pend_count.zero_()
            fb = getattr(self.policy_fn, "forward_counted_boards", None)
            if fb is not None:
                fb(self.cur_own, self.cur_opp, self._pend_idx, self.n_games, self._pend_count)
            else:
                self._policy_counted(self._policy_in[:self.n_games], self._pend_count)
        torch.cuda.synchronize()
        if self.lookahead:
            self._flush_lookahead(0)  # (queues empty: allocations and one-time setup only)
            self._flush_lookahead(1)
            if self.value_ahead:
                self._flush_value_ahead(0)
                with torch.cuda.stream(self._la_side):
                    self._flush_value_ahead(1)
            torch.cuda.synchronize()
        if self.async_steps:
            # the asynchronous step's own entry points, once, on empty queues and no game rolled
            self._a_wait.zero_()
            self._a_done.zero_()
            self._a_roll.zero_()
            self._a_fq_count.zero_()
            self._a_nsims.zero_()
            self._step_async(self._g_own, self._g_opp, torch.zeros_like(self._g_active))
            torch.cuda.synchronize()
        self._graph_long = None
        if self.lookahead and self.graph_blocks > 1:
            # the same block several times over: a replay costs tens of microseconds on the
            # device whatever it holds, so long searches replay the long graph and finish with
            # the one-block graph
            self._graph_long = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self._graph_long):
                for b in range(self.graph_blocks):
                    self._lookahead_block(self._g_own, self._g_opp, self._g_active, None, async_=self.async_steps,
                                          last=b + 1 == self.graph_blocks)
        self._graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._graph):
            if self.lookahead:
                # 2 K playouts (or steps) and the policy batches of the leaves they queue: ONE replay
                self._lookahead_block(self._g_own, self._g_opp, self._g_active, None, async_=self.async_steps)
            else:
                self._select(self._g_own, self._g_opp, self._g_active, True)
                self._expand_pending_counted(self._g_own, self._g_opp, self._g_active)
                self._evaluate_and_backup(self._g_active, stream_id=0, stream_id_dev=self._sim_dev,
                                          counter=self._sim_dev)

    def _search_graph(self, own, opp, active, n_sims, n_active):
        key = self._graph_state()
        if self._graph is None or key != self._graph_key:
            # first use, or the weights / rollout table changed since the capture (training
            # between searches, load_npz): the old graph holds pointers to freed layouts
            self._graph = None
            self._capture()
            self._graph_key = key
        self._g_own.copy_(own)
        self._g_opp.copy_(opp)
        self._g_active.copy_(active)
        self._sim_dev.fill_(self.sim_counter - (1 << 32) if self.sim_counter >= (1 << 31)
                            else self.sim_counter)
        if self.lookahead:
            block = 2 * self.lookahead
            n_blocks = n_sims // block
            if self._graph_long is not None:
                for _ in range(n_blocks // self.graph_blocks):
                    self._graph_long.replay()
                n_blocks %= self.graph_blocks
            for _ in range(n_blocks):
                self._graph.replay()
            # the same launches, not captured
            self._lookahead_tail(self._g_own, self._g_opp, self._g_active, n_sims % block, None)
        else:
            for _ in range(n_sims):
                self._graph.replay()
        self.sim_counter = (self.sim_counter + n_sims) & 0xFFFFFFFF
        self.n_leaf_evals += n_active * n_sims

    def _search_async(self, own, opp, active, n_sims, n_active):
        """n_sims playouts per active game as game-asynchronous steps: blocks of 2 K steps (one
        graph replay each, or the same launches eagerly) until every game has completed its
        playouts.  The number of steps depends on how often the games met fresh leaves, so the
        host reads one word back after the expected number of blocks and adds blocks while a
        game is behind; steps after the last game has finished do nothing."""
        if self.use_graph:
            key = self._graph_state()
            if self._graph is None or key != self._graph_key:
                self._graph = None
                self._capture()
                self._graph_key = key
            self._g_own.copy_(own)
            self._g_opp.copy_(opp)
            self._g_active.copy_(active)
            own, opp, act = self._g_own, self._g_opp, self._g_active
        else:
            act = active
        self._a_wait.zero_()
        self._a_done.zero_()
        self._a_roll.zero_()
        self._a_fq_count.zero_()
        self._a_nsims.fill_(n_sims)
        self._sim_dev.fill_(self.sim_counter - (1 << 32) if self.sim_counter >= (1 << 31) else self.sim_counter)
        block = 2 * self.lookahead
        want = self._async_hint.get(n_sims, n_sims + (self.async_parts - 1) * (n_sims // 5 + 1))
        steps = 0
        checks = 0
        while True:
            n_blocks = max(1, -(-(want - steps) // block))
            steps += n_blocks * block
            if self.use_graph:
                if self._graph_long is not None:
                    for _ in range(n_blocks // self.graph_blocks):
                        self._graph_long.replay()
                    n_blocks %= self.graph_blocks
                for _ in range(n_blocks):
                    self._graph.replay()
            else:
                for _ in range(n_blocks):
                    self._lookahead_block(own, opp, act, None, async_=True)
            checks += 1
            behind = bool(((self._a_done < n_sims) & (act != 0)).any().item())   # the search's host sync
            if not behind:
                break
            want = steps + block
        # one check: the estimate was enough (try one block less next time); more: remember the need
        self._async_hint[n_sims] = max(n_sims, steps - block) if checks == 1 else steps
        self.n_steps += steps
        self._lookahead_tail(own, opp, act, 0, None)   # the last group's policy batch: both queues end empty
        self.sim_counter = (self.sim_counter + n_sims) & 0xFFFFFFFF
        self.n_leaf_evals += n_active * n_sims

    def _search_persistent(self, own, opp, active, n_sims, n_active, root=None, turn=0):
        """n_sims playouts per active game as ONE launch (iago_mcts_search_persistent).  root (a RootRule): its draw of
        turn `turn` first, then the launch under it."""
        if root is None:
            self._launch_persistent(own, opp, active, n_sims)
        else:
            root.draw(self, own, opp, active, turn)
            self._launch_persistent(own, opp, active, n_sims, root=root)
        self.sim_counter = (self.sim_counter + n_sims) & 0xFFFFFFFF
        self.n_leaf_evals += n_active * n_sims

    def _launch_persistent(self, own, opp, active, n_sims, rules=NO_RULES, game=None, park=None, root=None):
        """iago_mcts_search_persistent: one search from the roots (own, opp), or -- game = dict(max_turns, own,
        opp, n_turns, rec_own, rec_opp, rec_valid, rec_move, rec_pi) -- whole self-play games under `rules` (a
        PlayRules).  park = dict(parked, stones, pass_flg), given with rules.solve_empties: those games handed over at
        that many empties (iago_mcts_search_park); rules.explore_turns: their moves of the turns below it drawn from the
        visit counts (iago_mcts_search_explore, which carries the hand-over); rules.playout_cap: their searched turns
        full or fast (iago_mcts_search_cap, which carries the other two).  root (a search's RootRule, else `rules`' own;
        never with `game`): RootRule.launch.  The role split where it is set up, else the single launch."""
        a, keep = self._search_args(own, opp, active, n_sims, game)
        root = root or RootRule.of(rules)
        ev = getattr(self, "launch_events", None)   # (bench.py: HIP event pairs around the launches, on their stream)
        if ev is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        k = None
        if park is not None:
            k = _lib.SearchParkArgs()
            k.park_empties = int(rules.solve_empties)
            k.parked, k.stones, k.pass_flg = park["parked"].data_ptr(), park["stones"].data_ptr(), park["pass_flg"].data_ptr()
        if self.wave_entry:
            if game is not None:
                raise ValueError("whole games in one launch are not available to the wave search (the turn loop is)")
            w = _lib.SearchWaveArgs()
            w.width, w.vloss, w.timing = self.wave, self.virtual_loss, self.wave_timing.data_ptr()
            self._wave_active = active
            check(_lib.lib().iago_mcts_search_wave(C.byref(a), C.byref(w), _stream()), "iago_mcts_search_wave")
        elif root is not None:
            root.launch(self, a, n_sims, game)
        elif rules.playout_cap is not None:
            ops.search_cap(a, *rules.playout_cap, explore_turns=rules.explore_turns, streams=self._split, park=k)
        elif rules.explore_turns:
            ops.search_explore(a, rules.explore_turns, streams=self._split, park=k)
        elif k is not None:
            k.streams = self._split
            check(_lib.lib().iago_mcts_search_park(C.byref(a), C.byref(k), _stream()), "iago_mcts_search_park")
        elif self._split is not None:
            check(_lib.lib().iago_mcts_search_split(C.byref(a), self._split, _stream()), "iago_mcts_search_split")
        else:
            check(_lib.lib().iago_mcts_search_persistent(C.byref(a), _stream()), "iago_mcts_search_persistent")
        if ev is not None:
            e1.record()
            ev.append((e0, e1))
        self._ps_keep = keep + (park,)   # alive until the next launch

    def _search_args(self, own, opp, active, n_sims, game=None):
        """The iago_mcts_search_args of a launch of the persistent search (own, opp, active, n_sims, game: as
        _launch_persistent takes them) and what they point to: (args, keep) -- the caller holds `keep` until the launch
        has run."""
        if self.rollout_hook is not None:
            raise ValueError("rollout_hook is not available in the persistent search (z_log_rows records the z)")
        ps = self._ps
        sid = self.sim_counter - (1 << 32) if self.sim_counter >= (1 << 31) else self.sim_counter
        ro = ops.rollout_prepare(self.cur_own, self.cur_opp, self.rollout_weights, seed=self.seed,
                                 id_base=self.game_id_base, stream_id=sid, out=self._rollout_out)
        with torch.no_grad():
            va, keep_v = self.value_fn.search_args(ps["wg_own"], ps["wg_opp"], ps["wg_v"])
            pa, keep_p = self.policy_fn.search_args(ps["wg_own"], ps["wg_opp"], ps["wg_probs"])
        a = _lib.MctsSearchArgs()
        a.tree = C.addressof(self.tree.c)
        if own is not None:
            a.root_own, a.root_opp = own.data_ptr(), opp.data_ptr()
        a.active = active.data_ptr()
        a.c_puct, a.lmbda, a.n_thr, a.n_sims = self.c_puct, self.lmbda, self.n_thr, int(n_sims)
        a.net_workgroups, a.time_limit_ms = self.net_workgroups, self.time_limit_ms
        a.games_per_workgroup = (self.games_per_workgroup | (_lib.SEARCH_CHAIN_SKIP if self.chain_skip else 0)
                                 | (_lib.SEARCH_NEGAMAX if self.backup == "negamax" else 0)
                                 | (_lib.SEARCH_PUCT_AZ if self.selection == "alphazero" else 0))
        a.pace_margin = self.pace_margin
        a.max_cus = self.max_cus
        a.value, a.policy, a.rollout = C.addressof(va), C.addressof(pa), C.addressof(ro.args)
        a.cur_node, a.cur_own, a.cur_opp = self.cur_node.data_ptr(), self.cur_own.data_ptr(), self.cur_opp.data_ptr()
        a.path, a.path_stride = ps["path"].data_ptr(), self.PATH_STRIDE
        a.done, a.roll, a.leaf_value = ps["done"].data_ptr(), ps["roll"].data_ptr(), self.leaf_value.data_ptr()
        if self.z_log is not None:
            a.z_log, a.z_log_n, a.z_log_rows = self.z_log.data_ptr(), self.z_log_n.data_ptr(), self.z_log.shape[0]
        a.q_slots, a.ctl = ps["q_slots"].data_ptr(), ps["ctl"].data_ptr()
        a.rep_v, a.rep_p, a.totals = ps["rep_v"].data_ptr(), ps["rep_p"].data_ptr(), ps["totals"].data_ptr()
        a.stats = self.stats.data_ptr() if self.stats is not None else None
        a.wg_own, a.wg_opp = ps["wg_own"].data_ptr(), ps["wg_opp"].data_ptr()
        if game is not None:
            a.max_turns = int(game["max_turns"])
            # (a whole game of 400-playout searches takes seconds; IAGO_PERSISTENT_GAME_LIMIT_MS: the lab's shorter limit)
            a.time_limit_ms = max(self.time_limit_ms, int(os.environ.get("IAGO_PERSISTENT_GAME_LIMIT_MS", "60000")))
            a.games_total = int(game.get("games_total", 0))
            if a.games_total:   # (a stream: the limit of a batch of whole games per batch's worth of games)
                a.time_limit_ms = min(a.time_limit_ms * -(-a.games_total // self.n_games), 0x7FFFFFFF)
            a.game_own, a.game_opp, a.n_turns = game["own"].data_ptr(), game["opp"].data_ptr(), game["n_turns"].data_ptr()
            a.rec_own, a.rec_opp = game["rec_own"].data_ptr(), game["rec_opp"].data_ptr()
            a.rec_valid, a.rec_move, a.rec_pi = (game["rec_valid"].data_ptr(), game["rec_move"].data_ptr(),
                                                 game["rec_pi"].data_ptr())
        if self._vtable is not None:
            a.vtable, a.vtable_slots = self._vtable.data_ptr(), self._vtable.numel() // 4
        if getattr(self, "trace", None) is not None:   # (diagnostic: tools/exp_persistent_trace.py)
            a.trace, a.trace_rows = self.trace.data_ptr(), self.trace.shape[0]
        return a, (keep_v, keep_p, ro, va, pa, own, opp, active, game)

    def reserve_net_rows(self, workgroups):
        """Rows of wg_own / wg_opp (four per workgroup) for a launch of `workgroups` workgroups that may all walk this
        engine's nets -- more than its own grid when the launch is an arena's (ops.search_arena)."""
        ps, rows = self._ps, 4 * int(workgroups)
        if ps["wg_own"].numel() < rows:
            kw = dict(device=ps["wg_own"].device)
            ps.update(wg_own=torch.zeros(rows, dtype=torch.int64, **kw), wg_opp=torch.zeros(rows, dtype=torch.int64, **kw),
                      wg_v=torch.zeros(rows, dtype=torch.float32, **kw),
                      wg_probs=torch.zeros((rows, 64), dtype=torch.float32, **kw))

    def _forget_stale_values(self):
        """The stored values belong to the weights that computed them: once the value net's parameters have changed,
        the values in the nodes and the position table are forgotten.  Before every launch that reads them."""
        if not self.value_cache:
            return
        key = tuple((q.data_ptr(), q._version) for q in self.value_fn.parameters())
        if key != self._value_key:
            if self._value_key is not None:
                self.tree.v.fill_(float("nan"))
                if self._vtable is not None:
                    self._vtable.zero_()
            self._value_key = key

    def _noise_rows(self):
        """The root noise's counts rows, (n_games, 64) int16, one per slot (iago_root_noise.counts)."""
        rows = getattr(self, "_noise_counts", None)
        if rows is None:
            rows = self._noise_counts = torch.zeros((self.n_games, 64), dtype=torch.int16, device=self.cur_own.device)
        return rows

    def _gumbel_state(self):
        """What the Gumbel root search keeps on the device: the two tables (ops.gumbel_tables, uploaded once), the draws
        g and the rows n / q / logit of gumbel_rows(), (n_games, 64) each, one row per slot, and the schedules by (m,
        n_sims).  `last`: the rule of the last such search, which gumbel_move() finishes."""
        st = getattr(self, "_gumbel", None)
        if st is None:
            dev, B = self.cur_own.device, self.n_games
            st = self._gumbel = dict(
                tables=tuple(torch.from_numpy(np.array(t)).to(dev) for t in ops.gumbel_tables()), sched={}, last=None,
                g=torch.zeros((B, 64), dtype=torch.int32, device=dev), n=torch.zeros((B, 64), dtype=torch.int32, device=dev),
                q=torch.zeros((B, 64), dtype=torch.float32, device=dev),
                logit=torch.zeros((B, 64), dtype=torch.int32, device=dev))
        return st

    def _gumbel_sched(self, m, n_sims):
        """ops.gumbel_schedule(m, n_sims) on the device, built once per (m, n_sims)."""
        sched = self._gumbel_state()["sched"]
        if (m, n_sims) not in sched:
            sched[m, n_sims] = torch.from_numpy(ops.gumbel_schedule(m, n_sims)).to(self.cur_own.device)
        return sched[m, n_sims]

    def _backup_check(self, rules=NO_RULES):
        """backup="negamax" and selection="alphazero" are the persistent search's alone: a rollout hook (set after
        construction) would send search() and SelfPlayEngine's turns through the per-playout launches, whose rules are the
        reference's.  Refused where a search or a round of games begins, before anything is reset."""
        per_playout = not getattr(self, "persistent", False) or getattr(self, "rollout_hook", None) is not None
        if getattr(self, "backup", "reference") == "negamax" and per_playout:
            raise ValueError(_NEGAMAX_NEEDS)
        if getattr(self, "selection", "reference") == "alphazero" and per_playout:
            raise ValueError(_ALPHAZERO_NEEDS)
        if RootRule.of(rules) is not None:   # (likewise the root rule of a round of games)
            RootRule.of(rules).require(self)
        if rules.root_values and getattr(self, "backup", "reference") != "negamax":
            raise ValueError(_ROOT_VALUE_NEEDS)

    def search_counts(self, active):
        """Device tensor int64[2]: games in `active`, nodes of the fullest pool -- what search()
        reads back before it starts (a caller that batches its readbacks passes them in)."""
        return torch.stack([active.sum().to(torch.int64), self.tree.n_nodes.max().to(torch.int64)])

    def search(self, own, opp, active, n_sims, counts=None, check=True, root_noise=None, turn=0, forced_playouts=None,
               gumbel=None):
        """n_sims playouts from the current roots; (own, opp) = root positions
        with own = side to move; active: uint8 mask of participating games.
        counts: (games in `active`, nodes of the fullest pool) when the caller has read
        search_counts() back already; check=False: the error flags are not read back here (one
        host sync each) -- the caller reads error_flags() and calls raise_errors().
        root_noise = (alpha_256, eps_256[, draws]) (None, the default: off; the persistent engine only, else
        ValueError): the priors of every active root's children are mixed with the shares of the Polya urn of turn
        `turn` of game game_id_base + g (include/iago_hip_serving.h, iago_mcts_root_noise) for the whole of this search,
        once -- children the root has are rewritten before the first playout, a root that expands creates them mixed.
        forced_playouts = k_256 (None, the default: off; an int in [1, 4096], with root_noise only, else ValueError):
        forced playouts at the root of this search (include/iago_hip_serving.h, iago_mcts_search_forced) -- a root child
        with n >= 1 visits and stored prior p scores +inf in Node.select while 256 n^2 < k_256 p N, N the root's visits.
        pruned_visits() afterwards takes the forced visits out of the visit rows.
        gumbel = (m, c_scale_256[, c_visit]) (None, the default: off; the persistent engine under backup="negamax" and
        selection="alphazero" only, never with root_noise or forced_playouts, else ValueError): the Gumbel root search
        (include/iago_hip_serving.h, iago_mcts_search_gumbel) -- the trees of the games in `active` are RESET first (the
        rule needs fresh roots: no subtree reuse), then the draw of turn `turn` of game game_id_base + g, then the search
        in which the root serves the sequential-halving schedule of (m, n_sims).  gumbel_move() afterwards gives the
        halving's survivor and gumbel_rows() the rows the improved-policy target is made from (gumbel_targets)."""
        self._backup_check()
        root = root_rule(n_sims, root_noise, forced_playouts, gumbel, engine=self)
        n_active, used = (int(v) for v in (self.search_counts(active).tolist() if counts is None else counts))
        if n_active == 0:
            # (the playout counter advances all the same: a game's Philox streams are keyed by ITS turn and
            # playout, whatever the other games of the batch do at that turn)
            self.sim_counter = (self.sim_counter + n_sims) & 0xFFFFFFFF
            return
        self._forget_stale_values()
        if self.value_cache:
            # (the descent appends to the fresh-leaf list through this count and the backup clears
            # it: a playout aborted between the two must not leave a stale count behind)
            self._fresh_count.zero_()
        if self.lookahead:
            # the cached priors of queued leaves belong to the policy weights that computed them
            params = getattr(self.policy_fn, "parameters", None)
            key = tuple((q.data_ptr(), q._version) for q in params()) if params is not None else id(self.policy_fn)
            if key != self._policy_key:
                if self._policy_key is not None:
                    self._la_stale.fill_(True)
                    self._la_stale_any = True
                self._policy_key = key
            if self._la_stale_any:
                self._refresh_priors(own, opp, active)
        if root is not None and root.fresh:
            self.tree.reset(active)   # (nothing left to compact in the searched games)
        else:
            self._compact_if_half_full(used)
        if root is not None or (self.persistent and self.rollout_hook is None):
            self._search_persistent(own, opp, active, n_sims, n_active, root, turn)
        elif self.async_steps and self.rollout_hook is None:
            self._search_async(own, opp, active, n_sims, n_active)
        elif self.use_graph:
            self._search_graph(own, opp, active, n_sims, n_active)
        elif self.lookahead:
            block = 2 * self.lookahead
            ids = iter([(self.sim_counter + i) & 0xFFFFFFFF for i in range(n_sims)])
            for _ in range(n_sims // block):
                self._lookahead_block(own, opp, active, ids)
            self._lookahead_tail(own, opp, active, n_sims % block, ids)
            self.sim_counter = (self.sim_counter + n_sims) & 0xFFFFFFFF
            self.n_leaf_evals += n_active * n_sims
        else:
            for _ in range(n_sims):
                self.simulate(own, opp, active, n_active)
        if check:
            self.raise_errors(self.error_flags().tolist())

    def _compact_if_half_full(self, used):
        """Before a search: `used` = the nodes of the fullest pool."""
        if used > self.tree.capacity // 2 and used > self._live_after_compaction * 5 // 4:
            # a pool is half full: free the nodes that subtree reuse left behind (what the
            # reference's garbage collector does after MCTS.py:149-152) before this search adds
            # its own.  A pool that fills up all the same is reported below.  (Not again until
            # the pool has grown by a quarter over what the last pass left: a live tree that
            # itself fills half the pool would otherwise be re-laid before every search.)
            self.tree.compact()
            self.n_compactions += 1
            self._live_after_compaction = int(self.tree.n_nodes.max().item())

    def gave_up_word(self):
        """Device copy (no sync) of the persistent search's gave-up word, None for the other engines.  Every launch
        clears the word: a caller that launches again before it reads error_flags() keeps this and passes it there."""
        return self._ps["ctl"][3].to(torch.int64) if self.persistent else None

    def error_flags(self, gave_up_before=None):
        """Device tensor int64[5]: pools that overflowed, the look-ahead's error word, the saturation
        flags of the value and the policy net (0 where a net has none), the persistent search's
        gave-up word -- ORed with gave_up_before, an earlier launch's gave_up_word()."""
        dev = self.cur_own.device
        zero = torch.zeros((), dtype=torch.int64, device=dev)
        parts = [self.tree.overflow.sum().to(torch.int64),
                 self._la_error[0].to(torch.int64) if self.lookahead else zero]
        for fn in (self.value_fn, self.policy_fn):
            f = getattr(fn, "__dict__", {}).get("_ovf") if hasattr(fn, "check_saturation") else None
            parts.append(f.reshape(-1)[0].to(torch.int64) if f is not None and f.device == dev else zero)
        gave = self._ps["ctl"][3].to(torch.int64) if self.persistent else zero
        parts.append(gave if gave_up_before is None else gave | gave_up_before)
        return torch.stack(parts)

    def raise_errors(self, flags):
        """The errors of a search from the host copy of error_flags()."""
        overflow, err, sat_v, sat_p, gave_up = (int(x) for x in flags)
        if gave_up and self.wave_entry and self._wave_active is not None:
            # the trees of a wave search that gave up still count playouts in flight (vv): fresh roots for them
            self.tree.reset(self._wave_active)
        if gave_up:
            raise _lib.IagoError("the persistent search gave up at its clock limit (%d ms for a search, 60 s for whole games: a "
                                 "reply never came -- is another job on the device, or fewer CUs free than workgroups?%s); the "
                                 "trees are incomplete"
                                 % (self.time_limit_ms, "  This was the role split (two launches on CU-masked streams): "
                                    "split=0 / IAGO_SEARCH_SPLIT=0 selects the single launch" if self._split is not None else ""))
        if overflow != 0:
            raise _lib.IagoError("MCTS node pool exhausted (or a search path deeper than 512): "
                                 "raise `capacity` (%d nodes per game)" % self.tree.capacity)
        if err:
            self._la_error.zero_()
            raise _lib.IagoError("policy look-ahead: %s" % (
                "the queue overflowed" if err == 1 else
                "a leaf reached n_thr without cached priors (raise `lookahead_slots`, now %d per "
                "game; the look-ahead must be on from the reset of the trees and n_thr must "
                "not change)" % self._la[0].slots))
        for fn, flag in ((self.value_fn, sat_v), (self.policy_fn, sat_p)):
            if flag:
                fn.check_saturation()  # raises (and clears the flag): the split-f16 kernels clamp at 65000

    def enable_stats(self):
        self.stats = torch.zeros((self.n_games, 2), dtype=torch.int32, device=self.cur_own.device)

    def tree_bytes(self):
        """Algorithmic bytes moved on the tree arrays so far, for the 32-byte
        node records: the descent reads one record per level (the node's header) and one per child
        scored; the backup reads and writes (n_visits, Q) = 8 + 8 B per node of the path (the levels
        + the leaf itself)."""
        lv, ch = (int(x) for x in self.stats.to(torch.int64).sum(dim=0).tolist())
        sel = 32 * (lv + ch) + 32 * self.n_leaf_evals
        bak = 16 * (lv + self.n_leaf_evals)
        return {"select": sel, "backup": bak, "levels": lv, "children_scored": ch}

    def memory_bytes(self):
        """Device memory this engine holds, by part: the tree pools (32-byte node records;
        twice that once compact() has allocated its second pool), the look-ahead's
        prior cache ([game][slot][64] float32) and queues, the recorded paths, and the policy
        net's scratch for its multi-launch forward (network.SLPolicy.SPLIT3_SCRATCH_ROWS x 51,200 B
        = 205 MB per stream that calls it -- the search uses up to three: eager, capture, side
        stream -- bounded whatever n_games is; longer batches run in chunks)."""
        out = {"tree": self.tree.bytes()}
        if getattr(self.tree, "_scratch", None) is not None:
            out["tree_compaction_pool"] = out["tree"] + self.tree._order.numel() * 4
        if self.lookahead:
            out["prior_cache"] = self._la_cache.numel() * 4 + self._la_cache_seq.numel() * 4
            out["queues"] = sum(t.numel() * t.element_size() for q in self._la_queues for t in q.values())
            if self._la_path is not None:
                out["paths"] = self._la_path.numel() * 4
        if self.persistent:
            out["persistent_search"] = sum(t.numel() * t.element_size() for t in self._ps.values())
            if self._vtable is not None:
                out["position_table"] = self._vtable.numel() * 8
        if self.value_ahead:
            out["value_ahead"] = sum(t.numel() * t.element_size() for d in self._va_x + [self._va_rows] for t in d.values())
        pool = getattr(self.policy_fn, "__dict__", {}).get("_split3_scratch_pool", {})
        out["policy_scratch"] = sum(b.numel() for k, b in pool.items() if k != "retired") + \
            sum(b.numel() for b in pool.get("retired", ()))
        return out

    def best_move(self, active=None, want_visits=True):
        """argmax visit count of the root's children, first wins (MCTS.py:147)."""
        check(_lib.lib().iago_mcts_best_move(self.tree.ref(),
                                             _p(active) if active is not None else None,
                                             _p(self.move), _p(self.visits) if want_visits else None,
                                             _stream()), "iago_mcts_best_move")
        return self.move, self.visits

    def root_value(self, active=None):
        """(q16, n) of the roots as they stand after a search (ops.mcts_root_value): per game in `active` (None: every
        game) the root's value for the root's MOVER in Q16 -- rint(-root.q * 65536), saturated to +-2^30 -- and the root's
        visits, both (n_games,) int32; 0 and 0 for the other games.  For engines with backup="negamax" only (ValueError):
        there a node's Q is the value for the player who moved into it, so -root.q is the mover's; under the reference's
        rule the root's Q mixes both players' views and is no value.  The engine's own buffers: the next call overwrites
        them.  Nothing is read back; a NaN or saturated value raises a bit of the engine's root_value_flags word."""
        if getattr(self, "backup", "reference") != "negamax":
            raise ValueError(_ROOT_VALUE_NEEDS)
        st = getattr(self, "_root_value", None)
        if st is None:
            dev = self.move.device
            st = self._root_value = (torch.zeros(self.n_games, dtype=torch.int32, device=dev),
                                     torch.zeros(self.n_games, dtype=torch.int32, device=dev),
                                     torch.ones(self.n_games, dtype=torch.uint8, device=dev))
            self.root_value_flags = torch.zeros(1, dtype=torch.int32, device=dev)
        return ops.mcts_root_value(self.tree.ref(), st[2] if active is None else active, st[0], st[1],
                                   self.root_value_flags)

    def gumbel_move(self, active=None, gumbel=None):
        """The move of the last search(gumbel=) on the trees as they stand (ops.gumbel_finish): of the root's most
        visited children the first maximum of g + logit + sigma(q); one child or none: best_move's answer.  Also fills the
        rows gumbel_rows() hands out.  gumbel: the rule, None = the last such search's.  Returns the engine's move buffer:
        the next best_move / draw_move overwrites it."""
        st = self._gumbel_state()
        rule = st["last"] if gumbel is None else ops.gumbel_arg(gumbel)
        if rule is None:
            raise ValueError("gumbel_move: no search(gumbel=) has run on this engine")
        ops.gumbel_finish(self.tree.ref(), active, rule, st["tables"], st["g"], self.move, st["n"], st["q"], st["logit"])
        return self.move

    def gumbel_rows(self, active=None, gumbel=None):
        """(n, q, logit) of the last search(gumbel=), (n_games, 64) each, by cell: the root children's visits (int32),
        their values (float32, 0 where unvisited) and logit_q16 of their stored priors (int32, INT32_MIN off the root's
        children) -- what gumbel_targets takes.  The engine's own buffers (the next call overwrites them; the rows of games
        outside `active` are stale)."""
        self.gumbel_move(active, gumbel)
        st = self._gumbel_state()
        return st["n"], st["q"], st["logit"]

    def pruned_visits(self, active=None, forced_playouts=512):
        """The policy-target pruning of forced playouts (ops.prune_visits) on the trees as they stand: the (n_games, 64)
        int32 visit rows of the roots of the games in `active` (None: every game) with the forced visits taken out where
        PUCT would not have granted them, under k_256 = forced_playouts, the engine's c_puct and its selection rule (the
        scores' denominator).  The engine's own buffer: the next call overwrites it; the rows of games outside `active` are
        stale."""
        k = ops.forced_playouts_arg(forced_playouts, noise=True)   # (the rule reads trees: whatever search wrote them)
        rows = getattr(self, "_pruned_rows", None)
        if rows is None:
            rows = self._pruned_rows = torch.zeros((self.n_games, 64), dtype=torch.int32, device=self.move.device)
        if getattr(self, "selection", "reference") == "alphazero":
            return ops.prune_visits(self.tree.ref(), active, self.c_puct, k, rows, _lib.SEARCH_PUCT_AZ)
        return ops.prune_visits(self.tree.ref(), active, self.c_puct, k, rows)

    def draw_move(self, turn, active=None, want_visits=True):
        """best_move for exploring self-play: the move drawn in proportion to the visit counts of the root's children
        (ops.draw_move), game g under the id game_id_base + g at turn `turn` (an int: every game's)."""
        ids, turns = self._turn_ids(turn)
        ops.draw_move(self.tree.ref(), active, self.seed, ids, turns, self.move, self.visits if want_visits else None)
        return self.move, self.visits

    def _turn_ids(self, turn):
        """(the games' global ids game_id_base + g as their 32 bits, `turn` for every game): two (n_games,) int32."""
        ids = getattr(self, "_draw_ids", None)
        if ids is None or ids[0] != self.game_id_base:
            g = (torch.arange(self.n_games, dtype=torch.int64, device=self.move.device) + self.game_id_base) & 0xFFFFFFFF
            ids = self._draw_ids = (self.game_id_base, torch.where(g >= (1 << 31), g - (1 << 32), g).to(torch.int32),
                                    torch.zeros(self.n_games, dtype=torch.int32, device=self.move.device))
        ids[2].fill_(int(turn))
        return ids[1], ids[2]

    def cap_mask(self, turn, full_per_256):
        """The playout cap's decision for turn `turn` (an int: every game's): a fresh (n_games,) uint8, 1 where the turn
        is a fast one for game g under the id game_id_base + g (ops.playout_cap_mask)."""
        ids, turns = self._turn_ids(turn)
        return ops.playout_cap_mask(self.seed, ids, turns, full_per_256)

    def update_with_move(self, move, mask=None):
        """MCTS.update_with_move (MCTS.py:149-154); move int8 tensor, -1 = pass."""
        check(_lib.lib().iago_mcts_advance_root(self.tree.ref(),
                                                _p(mask) if mask is not None else None, _p(move),
                                                _stream()), "iago_mcts_advance_root")


class SelfPlayResult(object):
    """Training tuples of one self-play round, device resident.

    own/opp: (T, B) int64 positions before each searched move (own = mover),
    pi: (T, B, 64) int32 root visit counts, valid: (T, B) uint8 (1: the game searched and moved
    at that turn; 4: it searched a FAST turn of the playout cap, playout_cap; 3: the move is the exact endgame
    solver's, solve_empties; 0: a pass or no turn),
    move: (T, B) int8, score: (T, B) int8 the exact final disc difference from the mover's view on
    the solved rows (0 elsewhere), z: (B,) int8 result from colour 1's view,
    mover: (T,) colour to move at that turn (1 or 2)."""

    SCORE_RECORD = "score"   # the attribute that holds the `score` record
    # forced_playouts: (T, B, 64) int32 the RAW visit rows, where `pi` then holds the pruned ones (the same on every row
    # that was not forced); None without forced playouts
    pi_raw = None
    # solved_targets: (T, B) int64 the set of the optimal moves of every solved row (bit a: move a reaches `score`), 0 on
    # every other row; None without solved targets
    best = None
    # root_values: (T, B) int32 the root's value from the MOVER's view in Q16 on the searched rows (valid 1 or 4), 0 on
    # every other row, and (T, B) int32 the root's visits there; None without root values
    q = None
    q_visits = None

    def value_targets(self, lam_256=256, mix_256=0):
        """The Value net's targets of the games, (T, B) int32 in Q16 from the mover's view (ops.value_targets,
        iago_value_targets): the result z mixed with the recorded root values -- TD(lambda) returns along the game,
        lambda = lam_256 / 256, and mix_256 / 256 of the row's own value; a solved row's value is the sign of its exact
        score.  (256, 0) is 65536 z from the mover's view, (256, 128) the z-q average, (0, 0) one-step bootstrapping.
        0 where there is no searched or solved row.  Needs play(root_values=True): ValueError without the record."""
        if self.q is None:
            raise ValueError("value_targets: the games recorded no root values (play(root_values=True) records them)")
        return ops.value_targets(self.valid, self.q, getattr(self, self.SCORE_RECORD, None), self.z, self.mover,
                                 lam_256, mix_256)

    def tuples(self, value_target=None):
        """Flat (s, pi, z) rows of all searched moves (valid == 1); z from the mover's view.  With root values recorded
        (play(root_values=True)) also q, the root's value from the mover's view in Q16.  value_target = (lam_256,
        mix_256): also v, the rows' value_targets(lam_256, mix_256) (int32, Q16)."""
        return self._rows(1, True, value_target)

    def fast_tuples(self, value_target=None):
        """tuples() of the FAST turns of the playout cap (valid == 4): searched with n_fast playouts, so not policy
        targets -- the game's result still labels them (and so do their roots' values: q and v as in tuples())."""
        return self._rows(_lib.REC_FAST, True, value_target)

    def solved_tuples(self, value_target=None):
        """Flat rows of the moves the endgame solver played (valid == 3): own, opp, move, score (the exact final disc
        difference from the mover's view), z (from the mover's view), colour, game, turn.  Where the games recorded
        solved targets (play(solved_targets=True)) also best, the set of the row's optimal moves (int64, bit a: move a
        reaches the score; `move` is its lowest bit), and pi (rows, 64) int32 with 1 on every optimal move: the rows then
        have every column ReplayWindow.add and ReinforceTrainer.step_from_tuples(..., target="visits") take.
        value_target = (lam_256, mix_256): also v, the rows' value_targets(lam_256, mix_256)."""
        rows = self._rows(3, False, value_target)
        if self.best is not None:
            rows["best"] = self.best.reshape(-1)[self.valid.reshape(-1) == 3]
            cells = torch.arange(64, device=rows["best"].device)
            rows["pi"] = ((rows["best"].reshape(-1, 1) >> cells) & 1).to(torch.int32)
        return rows

    def _rows(self, kind, searched, value_target=None):
        m = self.valid.reshape(-1) == kind
        T, B = self.valid.shape
        sign = torch.tensor([1 if c == 1 else -1 for c in self.mover], dtype=torch.int8,
                            device=self.z.device).reshape(T, 1)
        zz = (self.z.reshape(1, B) * sign).reshape(-1)
        dev = self.z.device
        colour = torch.tensor(list(self.mover), dtype=torch.int8, device=dev).reshape(T, 1).expand(T, B)
        # (global game id, turn) of a row: the key that puts the gathered rows of any number of
        # ranks into ONE canonical order (train_rl.ReinforceTrainer.step_from_tuples)
        game = (torch.arange(B, dtype=torch.int32, device=dev) + int(getattr(self, "game_id_base", 0))).reshape(1, B)
        turn = torch.arange(T, dtype=torch.int32, device=dev).reshape(T, 1)
        rows = dict(own=self.own.reshape(-1)[m], opp=self.opp.reshape(-1)[m], z=zz[m], move=self.move.reshape(-1)[m],
                    colour=colour.reshape(-1)[m], game=game.expand(T, B).reshape(-1)[m],
                    turn=turn.expand(T, B).reshape(-1)[m])
        if searched:
            rows["pi"] = self.pi.reshape(-1, 64)[m]
            if self.q is not None:
                rows["q"] = self.q.reshape(-1)[m]
        else:
            rows["score"] = getattr(self, self.SCORE_RECORD).reshape(-1)[m]
        if value_target is not None:
            rows["v"] = self.value_targets(*value_target).reshape(-1)[m]
        return rows


_BAD_DRAW = ("a match's policy draw met NaN / inf / zero probability mass on the legal moves (numpy.random.choice "
             "raises there, game.py:102-104)")


class MatchResult(SelfPlayResult):
    """The games of SelfPlayEngine.play_match: PV-MCTS against the SL policy (game.py:96-145,246-262).  As a
    SelfPlayResult, with valid 1 where PV-MCTS searched, 2 where a move was played without a search (the policy's
    draw -- or the move of play_match's `opponent` --, or a final move that was the only one: pi is 0 there), 3 where
    PV-MCTS played the endgame solver's move (solve_empties), 5 where either colour played a random opening move
    (opening_turns), 0 for a pass or no turn; mcts_colour: (B,) int8, the colour PV-MCTS played in each game.  score()
    being the match's result, the (T, B) record of the solved rows' exact scores is `solved_score` here."""

    SCORE_RECORD = "solved_score"
    # the turns of a match against AlphaBeta(depth, split) whose jobs did not fit the launch's room, answered by the
    # unsplit launch (the same moves)
    split_overflows = 0

    def tuples(self):
        """SelfPlayResult.tuples() of the positions PV-MCTS searched (valid == 1) only."""
        full = self.valid
        try:
            self.valid = (full == 1).to(full.dtype)
            return SelfPlayResult.tuples(self)
        finally:
            self.valid = full

    def score(self):
        """PV-MCTS's results: dict(wins, draws, losses, n, win_rate), a draw counting 1/2."""
        z = self.z.to(torch.int32) * torch.where(self.mcts_colour == 1, 1, -1).to(torch.int32)
        wins, draws, losses = (int(v) for v in torch.stack([(z > 0).sum(), (z == 0).sum(), (z < 0).sum()]).tolist())
        n = wins + draws + losses
        return dict(wins=wins, draws=draws, losses=losses, n=n, win_rate=(wins + 0.5 * draws) / n if n else float("nan"))


def _end_turns(valid):
    """(B,) each game's end turn from its records valid (T, B): the books of game.py:117-142,253-255 as the one-launch
    path keeps them -- a stone per move, a pass after a pass ends the game, `while stone_num < 64` once per pair of
    turns."""
    T, B = valid.shape
    dev = valid.device
    stones = torch.full((B,), 4, dtype=torch.int32, device=dev)
    pass_flg = torch.zeros(B, dtype=torch.bool, device=dev)
    over = torch.zeros(B, dtype=torch.bool, device=dev)
    end = torch.full((B,), T, dtype=torch.int32, device=dev)
    for t in range(T):
        moved = valid[t] != 0
        passing = ~moved & ~over
        stones = torch.where(passing & pass_flg, torch.full_like(stones, 64), stones + moved.to(torch.int32))
        pass_flg = torch.where(over, pass_flg, passing)
        if t % 2 == 1:
            new = ~over & (stones >= 64)
            end = torch.where(new, torch.full_like(end, t + 1), end)
            over = over | new
    return end


def _solve_empties_arg(k):
    """solve_empties of play / play_stream / play_match: None, or an int in [0, 20] (as MCTS(solve_empties=) takes it)."""
    if k is None:
        return None
    if isinstance(k, bool) or not isinstance(k, numbers.Integral) or not 0 <= k <= _lib.ENDGAME_MAX_EMPTIES:
        raise ValueError("solve_empties must be None or an int in [0, %d], not %r" % (_lib.ENDGAME_MAX_EMPTIES, k))
    return int(k)


def _play_rules(n_sims, solve_empties=None, explore_turns=None, playout_cap=None, root_noise=None, forced_playouts=None,
                solved_targets=False, gumbel=None, root_values=False):
    """The PlayRules of play / play_stream / play_match / ArenaEngine.play from their caller's arguments, each refused
    where its own validator refuses it (forced_playouts: an int in [1, 4096], and only with root_noise).  Off is (None, 0,
    None, None, None): explore_turns is an int in the record.  solved_targets: a bool, True only with solve_empties.
    gumbel: (m, c_scale_256[, c_visit]), refused together with explore_turns, root_noise or forced_playouts.
    root_values: a bool."""
    noise = ops.root_noise_arg(root_noise)
    # (the Gumbel checks now; forced_playouts, where no gumbel excludes it, after the others below)
    root = root_rule(n_sims, noise, forced_playouts if gumbel is not None else None, gumbel, explore_turns, "explore_turns, ")
    if not isinstance(solved_targets, bool):
        raise ValueError("solved_targets must be a bool, not %r" % (solved_targets,))
    if solved_targets and solve_empties is None:
        raise ValueError("solved_targets records the solver's optimal moves: it needs solve_empties")
    if not isinstance(root_values, bool):
        raise ValueError("root_values must be a bool, not %r" % (root_values,))
    return PlayRules(_solve_empties_arg(solve_empties), ops.explore_turns_arg(explore_turns) or 0,
                     ops.playout_cap_arg(playout_cap, n_sims), noise, ops.forced_playouts_arg(forced_playouts, noise),
                     solved_targets, root and root.gumbel, root_values)


def _no_forced_playouts(forced_playouts, who):
    """play_match and the arena do not force: forced playouts live only in noised self-play (play / play_stream)."""
    if forced_playouts is not None:
        raise ValueError("%s: forced_playouts is not available (forced playouts live only in the noised self-play of "
                         "play / play_stream)" % who)


def _match_rules(opponent, opening_turns, paired, mcts_colour, B):
    """The MatchRules of play_match from its arguments: opponent None or an AlphaBeta, opening_turns an even int in
    [0, 16], paired a bool that needs an even B and no mcts_colour beside it."""
    if opponent is not None and not isinstance(opponent, AlphaBeta):
        raise ValueError("play_match: opponent must be None (the policy net) or an AlphaBeta(depth), not %r" % (opponent,))
    if opponent is not None:   # (a record made past AlphaBeta's own checks, _make or _replace)
        opponent = AlphaBeta(*opponent)
    e = opening_turns
    if isinstance(e, bool) or not isinstance(e, numbers.Integral) or not 0 <= e <= 16 or e % 2:
        raise ValueError("play_match: opening_turns must be an even int in [0, 16], not %r" % (e,))
    if not isinstance(paired, bool):
        raise ValueError("play_match: paired must be True or False, not %r" % (paired,))
    if paired and mcts_colour is not None:
        raise ValueError("play_match: paired sets mcts_colour (colour 1 in the first half of the games, 2 in the second): "
                         "pass one of the two")
    if paired and B % 2:
        raise ValueError("play_match: paired needs an even number of games, not %d" % B)
    return MatchRules(opponent, int(e), B // 2 if paired else B)


def _colour_arg(colour, B, dev, name, or_none=""):
    """A colour argument -- 1, 2 or a (B,) integer tensor of 1 / 2 -- as a (B,) int8 tensor of 1 / 2 on `dev`.  name:
    the argument as the messages call it ("play_match: mcts_colour"); or_none: "None, " where the caller takes None."""
    what = "%s is %s1, 2 or a (%d,) integer tensor of 1 / 2" % (name, or_none, B)
    if isinstance(colour, torch.Tensor):
        if tuple(colour.shape) != (B,) or colour.is_floating_point() or colour.is_complex():
            raise ValueError(what)
        col = colour.to(device=dev, dtype=torch.int8)
        if not bool(((col == 1) | (col == 2)).all()) or not torch.equal(col.to(colour.dtype).cpu(), colour.cpu()):
            raise ValueError("%s holds values other than 1 and 2" % name)
        return col
    if isinstance(colour, bool) or not isinstance(colour, numbers.Integral) or colour not in (1, 2):
        raise ValueError(what)
    return torch.full((B,), int(colour), dtype=torch.int8, device=dev)


class _Side(object):
    """One searching side of the turn loop (SelfPlayEngine._play_turns): an engine, its playouts per move and the colour
    it searches -- a (B,) int8 tensor of 1 / 2, None: both.  The loop keeps the side's turn on it: `mine` (bool) and
    `act` (uint8), the games it searches and moves in, and `counts`, search_counts(act) on the host; under a playout cap
    `full` / `fast`, act's two parts, with `counts` / `counts_fast` theirs and `gave_up` the full games' gave-up word;
    `move` / `visits`, its engine's best_move or draw_move."""

    def __init__(self, mcts, n_sims, colour=None):
        self.mcts, self.n_sims, self.colour = mcts, n_sims, colour
        self.gave_up = None


def _empties(own, opp):
    """(n,) int32: 64 - popcount(own | opp), the true count of empty squares (stone_num ignores handicap stones)."""
    cells = torch.arange(64, device=own.device)
    return 64 - (((own | opp).reshape(-1, 1) >> cells) & 1).sum(dim=1).to(torch.int32)


def gumbel_targets(rows, c_visit=_lib.GUMBEL_C_VISIT, c_scale_256=256, scale=65536):
    """The improved-policy target of the Gumbel root search from the rows of BatchedMCTS.gumbel_rows() -- (n, q, logit),
    (B, 64) each, or with leading dimensions of any shape -- in torch float64 on the rows' device: over the legal moves
    (logit != INT32_MIN), pi' = softmax(logit_q16 / 65536 + sigma(completed q^)) with sigma(x) = (c_visit + max n)
    (c_scale_256 / 256) x and q^ = (q + 1) / 2.  The completed q of a visited move is its q; of an unvisited legal move
    v_mix = (v0 + N wq) / (1 + N), N the sum of the visits, wq the mean q of the visited moves weighted by their priors p =
    exp(logit_q16 / 65536), and v0 = wq (the root's own value is not kept).  A root without a visited child keeps its prior,
    softmax(logit); a row without a legal move is 0.  Returns int32 rows round(scale pi'), the column ReplayWindow.add and
    ReinforceTrainer.step_from_tuples(target="visits") take."""
    n, q, logit = rows
    f64 = torch.float64
    legal = logit != -(1 << 31)
    zero = torch.zeros((), dtype=f64, device=n.device)
    lg = torch.where(legal, logit.to(f64) / 65536.0, zero)
    nn, qq = n.to(f64), q.to(f64)
    visited = legal & (n > 0)
    p = torch.where(visited, torch.exp(lg), zero)
    big_n = nn.sum(dim=-1, keepdim=True)
    psum = p.sum(dim=-1, keepdim=True)
    some = psum > 0
    wq = (p * qq).sum(dim=-1, keepdim=True) / torch.where(some, psum, torch.ones_like(psum))
    v_mix = (wq + big_n * wq) / (1.0 + big_n)
    q_hat = (torch.where(visited, qq, v_mix) + 1.0) / 2.0
    sigma = (float(c_visit) + nn.max(dim=-1, keepdim=True).values) * (float(c_scale_256) / 256.0) * q_hat
    x = lg + torch.where(some, sigma, zero)
    x = torch.where(legal, x, torch.full_like(x, -float("inf")))
    top = x.max(dim=-1, keepdim=True).values
    e = torch.where(legal, torch.exp(x - torch.where(top > -float("inf"), top, zero)), zero)
    tot = e.sum(dim=-1, keepdim=True)
    pi = e / torch.where(tot > 0, tot, torch.ones_like(tot))
    return torch.round(float(scale) * pi).to(torch.int32)


class SelfPlayEngine(object):
    """Whole games on the B boards of a BatchedMCTS, three ways.  play(): lockstep PV-MCTS self-play -- both colours
    search the shared tree, moves are the most visited children, passes advance the tree with -1 (game.py:117-142 turn
    structure, both sides driven by MCTS.get_move).  play_stream(): n_games such games through the B slots.
    play_match(): PV-MCTS against the SL policy (game.py --auto).  Each validates its rules once (_play_rules: a
    PlayRules) and hands them on as one value.  Two paths behind them, the same games record for record: ONE launch of
    the persistent search that walks every game through its own turns (_play_persistent, wherever
    _whole_games_in_one_launch allows it), and the turn loop (_play_turns: a search per searching side and ONE host
    readback per turn; self-play is one side that searches both colours, a match one side of one colour with the other
    colour's moves drawn from the policy net, ArenaEngine's games two sides), which is also the replay of a batch whose
    launch filled a pool up (n_replayed counts those)."""

    def __init__(self, mcts, max_turns=_lib.IAGO_MAX_TURNS):
        self.mcts = mcts
        self.B = mcts.n_games
        self.max_turns = max_turns
        self.n_replayed = 0   # batches replayed through the turn loop

    def _start_boards(self, n, handicap=None):
        """(own, opp) of n games at the opening; handicap: (n,) int64 bit masks of extra colour-2 stones."""
        dev = self.mcts.cur_own.device
        own = torch.full((n,), START_OWN, dtype=torch.int64, device=dev)
        opp = torch.full((n,), START_OPP, dtype=torch.int64, device=dev)
        return own, opp if handicap is None else opp | handicap

    def _new_records(self, B):
        """The record tensors of B games, max_turns rows each, by their SelfPlayResult names."""
        T, dev = self.max_turns, self.mcts.cur_own.device
        return dict(own=torch.zeros((T, B), dtype=torch.int64, device=dev),
                    opp=torch.zeros((T, B), dtype=torch.int64, device=dev),
                    pi=torch.zeros((T, B, 64), dtype=torch.int32, device=dev),
                    valid=torch.zeros((T, B), dtype=torch.uint8, device=dev),
                    move=torch.full((T, B), -1, dtype=torch.int8, device=dev),
                    score=torch.zeros((T, B), dtype=torch.int8, device=dev))

    def _finish(self, res, p1, p2, t, launches, game_turns=None):
        """What every result ends with: the header of a batch of t turns and its final boards (colour 1's stones,
        colour 2's), judged.  game_turns: (B,) the turn at which each game ended -- the one-launch path records them."""
        res.game_id_base = self.mcts.game_id_base
        res.n_turns, res.launches, res.game_turns = t, launches, game_turns
        res.mover = [1 if k % 2 == 0 else 2 for k in range(t)]
        res.z = ops.judge(p1, p2)
        res.final_p1, res.final_p2 = p1, p2
        return res

    def _play_persistent(self, n_sims, own, opp, record, rules, games_total=0, active=None, res=None):
        """The whole game of every board in ONE launch (iago_mcts_search_persistent with max_turns > 0): each
        game walks through its own turns -- search, most visited move, update_with_move, the stone, the books
        -- with no barrier between the games' turns.  Same moves, visit counts and results as the turn-by-turn
        loop below (tests/test_search_persistent_gpu.py).  games_total > 0: the games_total games of own / opp
        as a stream through the B slots (play_stream).  active: (B,) uint8 kinds of game (play_match's codes), default
        all self-play; res: the result object to fill (default a SelfPlayResult).  None: a pool filled up.
        rules (a PlayRules): solve_empties = k: TWO launches -- the games hand over at their first turn of at most k
        empties (iago_mcts_search_park), then iago_play_endgame plays every game to its end under perfect play, into the
        same records (valid 3, score; with solved_targets iago_play_endgame_moves, and the record best), and the one
        readback follows both.  explore_turns > 0: the searched moves of the
        turns below it are drawn from the visit counts, in the launch (iago_mcts_search_explore).  playout_cap =
        (n_fast, full_per_256): every searched turn is full or fast, in the launch (iago_mcts_search_cap).  (Games with
        root_noise do not come here: _one_launch.)"""
        m, T = self.mcts, self.max_turns
        solve_empties, cap = rules.solve_empties, rules.playout_cap
        B = games_total or self.B        # (the result's columns: one per game)
        dev = own.device
        rec = self._new_records(B)
        g = dict(max_turns=T, games_total=games_total, own=own, opp=opp, n_turns=torch.zeros(B, dtype=torch.int32, device=dev),
                 **{"rec_" + k: v for k, v in rec.items()})
        if rules.solved_targets:   # (the play-out's own record: the search's launch does not see it)
            rec["best"] = torch.zeros((T, B), dtype=torch.int64, device=dev)
        if active is None:
            active = torch.ones(self.B, dtype=torch.uint8, device=dev)
        m._forget_stale_values()
        # (what the launch accumulates into, in case a pool fills up and the batch is replayed turn by turn)
        keep = [(t, t.clone()) for t in (m._ps["totals"], m.z_log_n, m.stats) if t is not None]
        park = None
        if solve_empties is not None:
            park = dict(parked=torch.zeros(B, dtype=torch.uint8, device=dev),
                        stones=torch.zeros(B, dtype=torch.int32, device=dev),
                        pass_flg=torch.zeros(B, dtype=torch.uint8, device=dev))
        m._launch_persistent(None, None, active, n_sims, rules, game=g, park=park)
        out = None
        if park is not None:
            # (own / opp / n_turns: a parked game's position and turn in, its final position and turn count out)
            out = ops.play_endgame(own, opp, g["n_turns"], park["stones"], park["pass_flg"], park["parked"], max_turns=T,
                                   max_empties=solve_empties, records={k: rec[k] for k in ("own", "opp", "valid", "move", "score")
                                                                       + (("best",) if rules.solved_targets else ())},
                                   check_result=False, **({"best": True} if rules.solved_targets else {}))
        ctl = m._ps["ctl"]
        back = _read_back(dict(
            flags=m.error_flags(), no_children=ctl[4], turns=g["n_turns"].max(), full_rows=(rec["valid"] == 1).sum(),
            net_workgroups=ctl[7], bad_draw=ctl[_lib.CTL_BAD_DRAW], endgame_ctl=out and out["ctl"],
            unfinished=out and (out["finished"] != park["parked"]).sum(),
            fast_rows=(rec["valid"] == _lib.REC_FAST).sum() if cap is not None else None))
        m.net_workgroups_launched = back["net_workgroups"]
        overflow, _, _, _, gave_up = back["flags"]
        if overflow and not gave_up:
            # a pool filled up (the launch cannot compact): nothing of this attempt counts
            for t, was in keep:
                t.copy_(was)
            return None
        m.raise_errors(back["flags"])
        if back["no_children"]:
            raise ValueError("a searched root has no children: n_sims is below the expansion threshold n_thr")
        if back["bad_draw"]:
            raise _lib.IagoError(_BAD_DRAW)
        if park is not None:
            ops.check_play_endgame(back["endgame_ctl"] + [back["unfinished"]], out, solve_empties, ops.ENDGAME_TIME_LIMIT_MS)
        t = back["turns"]
        m.sim_counter = (m.sim_counter + t * n_sims) & 0xFFFFFFFF
        m.n_leaf_evals += back["full_rows"] * n_sims + (0 if cap is None else back["fast_rows"] * cap[0])
        # a game's boards after n_turns[g] swaps of sides; colour 1's stones are `own` after an even number
        even = (g["n_turns"] % 2 == 0)
        p1, p2 = torch.where(even, own, opp), torch.where(even, opp, own)
        res = self._finish(SelfPlayResult() if res is None else res, p1, p2, t, 1 if park is None else 2,
                           game_turns=g["n_turns"])
        if record:
            turn = torch.arange(t, device=dev).reshape(t, 1)
            played = turn < g["n_turns"].reshape(1, B)
            # (the turn-by-turn loop records a finished game's boards, still swapping sides, until the last game
            # of the batch is over: the same rows here)
            tw = (turn % 2 == 0)
            res.own = torch.where(played, rec["own"][:t], torch.where(tw, p1.reshape(1, B), p2.reshape(1, B)))
            res.opp = torch.where(played, rec["opp"][:t], torch.where(tw, p2.reshape(1, B), p1.reshape(1, B)))
            res.valid, res.move, res.pi = rec["valid"][:t], rec["move"][:t], rec["pi"][:t]
            setattr(res, res.SCORE_RECORD, rec["score"][:t])
            if rules.solved_targets:
                res.best = rec["best"][:t]
        return res

    def _whole_games_in_one_launch(self, n_sims):
        m = self.mcts
        return (getattr(m, "persistent", False) and m.rollout_hook is None and not getattr(m, "wave_entry", False)
                and os.environ.get("IAGO_PERSISTENT_GAMES", "1") != "0"
                and 2 * m.tree.capacity >= suggest_capacity(n_sims, m.n_thr, moves=min(self.max_turns, 64)))

    def _one_launch(self, n_sims, n, handicap, record, rules, applies=True, **kw):
        """Fresh trees, then the n games in one launch (_play_persistent(rules, **kw)) wherever the persistent search
        applies (and the caller's own condition does) and the pools can hold a whole game without compaction.  None where it
        does not -- and where a pool filled up all the same (n_replayed) -- with the trees fresh for the caller's
        fallback, whose searches (one launch per turn) compact a pool that is half full.  Same games either way."""
        m = self.mcts
        m.tree.reset()
        # (a root rule draws per turn by a launch of its own, ops.root_noise or ops.gumbel_draw -- the turn loop; so do
        # root values, read per turn by ops.mcts_root_value: the whole-game launch does not record them)
        if not (applies and RootRule.of(rules) is None and not rules.root_values and self._whole_games_in_one_launch(n_sims)):
            return None
        res = self._play_persistent(n_sims, *self._start_boards(n, handicap), record, rules, **kw)
        if res is None:
            self.n_replayed += 1
            m.tree.reset()
        return res

    def _search_sides(self, sides, own, opp, rules):
        """The turn's searches, one side after the other (check=False: the loop reads every side's flags back).  Under a
        playout cap TWO searches per side from the same sim_counter -- a fast turn is the first n_fast playouts of the
        full turn's search: the same Philox streams -- and the counter n_sims on, once.  A root rule goes with the search
        (of a cap's two with the full games' alone) beside the side's turn.  Returns 1: `launches` counts the turns."""
        root = RootRule.of(rules)
        for s in sides:
            m = s.mcts
            kw = {} if root is None else dict({k: v for k, v in root._asdict().items() if v is not None}, turn=s.turn)
            if rules.playout_cap is None:
                m.search(own, opp, s.act, s.n_sims, counts=s.counts, check=False, **kw)   # (sim_counter: + n_sims whoever searched)
                continue
            s0 = m.sim_counter
            if s.counts[0] + s.counts_fast[0] > 0:
                m._compact_if_half_full(int(s.counts[1]))   # (once, for both searches: used = 0 keeps them from it)
            m.search(own, opp, s.full, s.n_sims, counts=(s.counts[0], 0), check=False, **kw)
            # (the fast games' launch clears the gave-up word of the full games': kept on the device for the readback)
            s.gave_up = m.gave_up_word()
            m.sim_counter = s0
            m.search(own, opp, s.fast, rules.playout_cap[0], counts=(s.counts_fast[0], 0), check=False)
            m.sim_counter = (s0 + s.n_sims) & 0xFFFFFFFF
        return 1

    def _play_turns(self, sides, own, opp, record, res, rules, policy_moves=False, search=None, match=None):
        """The games from (own, opp) turn by turn into res, in lockstep: per turn a search from every root that a side
        searches, the move, the books, and ONE host readback.  sides: the _Side's that search -- one of colour None is
        self-play (every active game searched), one of a colour with policy_moves is play_match (the other colour's
        moves drawn from the first side's policy net, a final only move forced: searched by nobody), two of
        complementary colours are the arena's agents; every side's tree follows every move.  search(sides, own, opp,
        rules) -> launches runs the turn's searches: by default _search_sides, the one thing ArenaEngine replaces;
        res.launches is the sum of what it returns.  rules (a PlayRules): solve_empties = k: a game that would search at
        a position of at most k empties leaves the search mask; the solver (ops.solve_endgame, EXACT: one launch per turn
        for all such games) gives its move, recorded with valid 3 and the exact score, and its flags join the turn's
        readback; with solved_targets ops.solve_endgame_moves(moves="best") instead, and the record best.
        explore_turns: the searched moves of the turns below it are drawn from the visit counts
        (BatchedMCTS.draw_move) instead of best_move's.  playout_cap = (n_fast, full_per_256): the turn's full games
        (BatchedMCTS.cap_mask) search n_sims playouts, its fast ones n_fast, recorded with valid 4 (_search_sides).
        forced_playouts = k_256: the games the noised search forced (every searched one, under a cap the full ones) record
        their pruned visit row (BatchedMCTS.pruned_visits) in pi and the raw row in pi_raw; every other row is the raw one
        in both.  The move comes from the raw counts.  match (a MatchRules, with policy_moves): the other colour's
        moves are ops.alphabeta_moves' where it names an opponent (one launch per turn, its `done` flags in the turn's
        readback), still recorded with valid 2; at the turns below its opening_turns nobody searches or draws and both
        colours play ops.random_moves' move, recorded with valid 5 (REC_OPENING).  An opponent with a split is launched
        with room for B x ALPHABETA_JOBS_PER_ROOT[split] jobs; a turn whose jobs do not fit is answered by the unsplit launch
        (chosen on the device) and counted in res.split_overflows from the turn's readback."""
        B, T, dev = self.B, self.max_turns, own.device
        k, cap = rules.solve_empties, rules.playout_cap
        opponent, opening_turns = (match.opponent, match.opening_turns) if match is not None else (None, 0)
        search = search or self._search_sides
        stone_num = torch.full((B,), 4, dtype=torch.int32, device=dev)  # game.py:32
        pass_flg = torch.zeros(B, dtype=torch.uint8, device=dev)
        done = torch.zeros(B, dtype=torch.uint8, device=dev)
        rec = self._new_records(B) if record else None
        root = RootRule.of(rules)
        targets = record and root is not None and root.targets   # (the rule's own policy target in pi, the raw row in pi_raw)
        if targets:
            rec["pi_raw"] = torch.zeros_like(rec["pi"])
        if record and rules.solved_targets:
            rec["best"] = torch.zeros((T, B), dtype=torch.int64, device=dev)
        values = record and rules.root_values   # (the roots' values and visits of the searched rows: q, q_visits)
        if values:
            rec["q"] = torch.zeros((T, B), dtype=torch.int32, device=dev)
            rec["q_visits"] = torch.zeros((T, B), dtype=torch.int32, device=dev)
        legal = ops.legal_moves(own, opp)
        active = (legal != 0).to(torch.uint8)
        legal_next, active_next = torch.empty_like(legal), torch.empty_like(active)
        none = torch.full((B,), -1, dtype=torch.int8, device=dev)
        if policy_moves:
            m0 = sides[0].mcts
            cells = torch.arange(64, device=dev)
            key, pf = m0.seed ^ _lib.MATCH_SEED_XOR, m0.policy_fn
        if k is not None:
            # (the fewest empties any game starts with: a turn takes at most one, so before turn least - k no game can be
            # at k empties and nothing is launched for the solver)
            least = int(_empties(own, opp).min().item())
        if k is not None or opponent is not None:
            full_board, no_board = torch.full_like(own, -1), torch.zeros_like(own)

        def movers(t):
            """Who moves at turn t: every side's `mine` / `act` (under a cap `full` / `fast` too).  Returns the games
            whose move the policy (or the match's opponent) draws, those whose move is forced, those whose move the
            solver plays, those that play a random opening move (None where there are none of the kind) and, as device
            values by name, the counts the turn's searches start from."""
            everyone = active.bool()
            drawn = forced = sol = at_end = None
            # (an opening turn: every game that can move plays a random move, nobody searches or draws)
            opening = everyone if t < opening_turns else None
            on = everyone if opening is None else torch.zeros_like(everyone)
            if policy_moves:
                # game.py:97-98: the only move of the last empty square, either side, no search
                forced = on & (stone_num > 62) & ((legal & (legal - 1)) == 0)
                drawn = on & ~forced
            if k is not None and least - t <= k:
                at_end = _empties(own, opp) <= k
            counts = {}
            for i, s in enumerate(sides):
                mine = on if s.colour is None else on & (s.colour == (1 if t % 2 == 0 else 2))
                if policy_moves:
                    drawn, mine = drawn & ~mine, mine & ~forced
                if at_end is not None:
                    sol = mine & at_end if sol is None else sol | (mine & at_end)
                    mine = mine & ~at_end
                s.mine, s.act, s.turn = mine, active if mine is everyone else mine.to(torch.uint8), t
                s.ruled = s.act   # (the games a root rule searches: every searched one, under a cap the full ones)
                if cap is not None:
                    s.fast = s.mcts.cap_mask(t, cap[1]) & s.act
                    s.full = s.ruled = s.act ^ s.fast
                counts["counts", i] = s.mcts.search_counts(s.ruled)
                if cap is not None:
                    counts["counts_fast", i] = s.mcts.search_counts(s.fast)
            return drawn, forced, sol, opening, counts

        def start_from(back):
            for i, s in enumerate(sides):
                s.counts, s.counts_fast = back["counts", i], back.get(("counts_fast", i))

        t, launched, split_overflows = 0, 0, 0
        drawn, forced, sol, opening, counts = movers(t)
        start_from(_read_back(counts))
        while t < T:
            # ONE readback per turn (below): every side's flags of this turn's search, the checks of its moves, the
            # end-of-game test and the counts the next searches start from
            launched += search(sides, own, opp, rules)
            for s in sides:
                s.move, s.visits = s.mcts.draw_move(t, s.act) if t < rules.explore_turns else s.mcts.best_move(s.act)
                if root is not None:   # (the rule's own move, written over best_move's in s.move: the engine's move buffer)
                    s.made = root.move(s.mcts, s.ruled, record)
                if values:   # (the engine's own buffers, 0 outside s.act: into the record at once; a game has one mover)
                    q, n = s.mcts.root_value(s.act)
                    rec["q"][t] += q
                    rec["q_visits"][t] += n
            if sol is not None:
                # (a game that is not solved here sends a full board: no search, no refusal)
                if rules.solved_targets:   # (the same score and move, and the set of the optimal moves)
                    ex = ops.solve_endgame_moves(torch.where(sol, own, full_board), torch.where(sol, opp, no_board),
                                                 mode="exact", moves="best", max_empties=k, check_result=False)
                else:
                    ex = ops.solve_endgame(torch.where(sol, own, full_board), torch.where(sol, opp, no_board), mode="exact",
                                           max_empties=k, check_result=False)
            mv = none
            ab = ab_over = None
            if policy_moves and opening is None:
                if opponent is not None:
                    # (a game that the opponent does not move in sends a full board: no search, no refusal)
                    ab = ops.alphabeta_moves(torch.where(drawn, own, full_board), torch.where(drawn, opp, no_board),
                                             opponent.depth, check_result=False, split=opponent.split,
                                             job_capacity=B * ALPHABETA_JOBS_PER_ROOT[opponent.split]
                                             if opponent.split else None)
                    if opponent.split:
                        # A turn whose jobs did not fit is answered by the unsplit launch: the same moves.  It is chosen
                        # on the device -- with the jobs in their room every game sends it a full board, one node --,
                        # so an overflow costs no readback of its own and never plays a wrong move.
                        ab_over = ab["ctl"][6] != 0
                        whole = ops.alphabeta_moves(torch.where(drawn & ab_over, own, full_board),
                                                    torch.where(drawn & ab_over, opp, no_board), opponent.depth,
                                                    check_result=False)
                        ab = {k: torch.where(ab_over, whole[k], ab[k]) for k in ("move", "done")}
                    draw = ab["move"]
                else:
                    with torch.no_grad():
                        if hasattr(pf, "forward_boards_split3"):
                            probs = pf.forward_boards_split3(own, opp)
                        else:
                            probs = pf(ops.encode_planes(own, opp))
                    draw = ops.sample_moves(probs.reshape(B, 64), torch.where(drawn, legal, torch.zeros_like(legal)),
                                            seed=key, id_base=m0.game_id_base, step=t, stream_id=0)
                only = ((legal.reshape(B, 1) >> cells) & 1).argmax(dim=1).to(torch.int8)
                mv = torch.where(drawn, draw, torch.where(forced, only, none))
            elif opening is not None:
                mv = torch.where(opening, ops.random_moves(own, opp, m0.seed, m0.game_id_base, match.id_mod, t), none)
            for s in reversed(sides):
                mv = torch.where(s.mine, s.move, mv)
            if sol is not None:
                mv = torch.where(sol, ex["move"], mv)
            if record:
                valid = pi = None
                for s in sides:   # (a game has one mover: the sides' rows do not overlap)
                    v = s.act if cap is None else s.act + (_lib.REC_FAST - 1) * s.fast
                    p = s.visits * s.act.reshape(B, 1).to(torch.int32)
                    valid, pi = (v, p) if valid is None else (valid | v, pi + p)
                if targets:
                    rec["pi_raw"][t] = pi
                    for s in sides:   # (the games the rule searched: its target for the visit row)
                        pi = torch.where(s.ruled.reshape(B, 1) != 0, root.target(s.mcts, s.ruled, s.made), pi)
                if policy_moves:
                    valid = valid + _lib.REC_DRAWN * (drawn | forced).to(torch.uint8)
                if opening is not None:
                    valid = valid + _lib.REC_OPENING * opening.to(torch.uint8)
                if sol is not None:
                    valid = valid + 3 * sol.to(torch.uint8)
                    rec["score"][t] = torch.where(sol, ex["score"], torch.zeros_like(ex["score"]))
                    if rules.solved_targets:
                        rec["best"][t] = torch.where(sol, ex["best"], torch.zeros_like(ex["best"]))
                rec["own"][t], rec["opp"][t], rec["valid"][t], rec["move"][t], rec["pi"][t] = own, opp, valid, mv, pi
            # game.py:84,108,140: the games not yet done -- less, in a match, the forced moves (game.py:107,113)
            live = ((done == 0) & ~forced).to(torch.uint8) if policy_moves else done ^ 1
            for s in sides:
                s.mcts.update_with_move(mv, live)
            # the move, stone_num / pass_flg, `while game.stone_num < 64` once per pair of turns
            # (game.py:117-142,253-255), the swap of sides, the next mover's legal moves
            ops.play_turn(own, opp, mv, active, stone_num, pass_flg, done, t % 2 == 1, legal_next, active_next)
            legal, legal_next = legal_next, legal
            active, active_next = active_next, active
            t += 1
            # (mv is -2 only where best_move found a searched root without children: a drawn move is -1 .. 64, a solved
            # one a legal move)
            checks = dict(no_children=(mv == -2).any(), all_done=done.all(),
                          bad_draw=(drawn & (draw == 64)).any() if policy_moves and opening is None else None,
                          unsolved=(ex["solved"] == 0).any() if sol is not None else None,
                          unfinished=(ab["done"] == 0).any() if ab is not None else None, split_overflow=ab_over,
                          bad_value=sum(s.mcts.root_value_flags[0] & _lib.ROOT_VALUE_NAN for s in sides) if values else None)
            drawn, forced, sol, opening, counts = movers(t)
            back = _read_back({**{("flags", i): s.mcts.error_flags(s.gave_up) for i, s in enumerate(sides)},
                               **checks, **counts})
            for i, s in enumerate(sides):
                s.mcts.raise_errors(back["flags", i])
            if back["no_children"]:
                # what max() over an empty children dict raises in MCTS.get_move (MCTS.py:147)
                raise ValueError("a searched root has no children: n_sims is below the expansion threshold n_thr")
            if back.get("bad_draw"):
                raise _lib.IagoError(_BAD_DRAW)
            if back.get("unsolved"):
                raise _lib.IagoError("solve_empties = %d: the endgame solver refused or did not finish a position at "
                                     "turn %d" % (k, t - 1))
            if back.get("bad_value"):
                for s in sides:
                    s.mcts.root_value_flags.zero_()
                raise _lib.IagoError("root_values: a searched root's value is NaN at turn %d" % (t - 1))
            if back.get("unfinished"):
                raise _lib.IagoError("play_match: the alpha-beta opponent (depth %d) did not finish a position at turn %d"
                                     % (opponent.depth, t - 1))
            split_overflows += int(back.get("split_overflow") or 0)
            if t % 2 == 0 and back["all_done"]:
                break
            start_from(back)
        if opponent is not None:
            res.split_overflows = split_overflows
        # colour 1's stones are `own` after an even number of turns
        p1, p2 = (own, opp) if t % 2 == 0 else (opp, own)
        self._finish(res, p1, p2, t, launched)
        if record:
            for name, v in rec.items():
                name = res.SCORE_RECORD if name == "score" else name
                if name is not None:   # (an ArenaResult keeps no score record)
                    setattr(res, name, v[:t])
        return res

    def play(self, n_sims, handicap=None, record=True, solve_empties=None, explore_turns=None, playout_cap=None,
             root_noise=None, forced_playouts=None, solved_targets=False, gumbel=None, root_values=False):
        """B self-play games; handicap: (B,) int64 bit masks of extra colour-2 stones.  Returns a SelfPlayResult.
        solve_empties = k (an int in [0, 20]; None, the default: off): a turn that would be searched at a position of
        at most k empties (64 - popcount(own | opp)) runs no search -- the move is the exact endgame solver's
        (iago_solve_endgame, EXACT: the lowest-indexed move reaching the best final disc difference), recorded with
        valid 3, pi 0 and the exact score from the mover's view in `score`, and played through update_with_move and the
        books like a searched move.  The games then end under perfect play: z is the game-theoretic value of every
        position from the first solved turn on.  sim_counter advances by n_sims per turn all the same; n_leaf_evals
        counts the valid == 1 rows.  Where whole games run in one launch they hand over at k empties and ONE more launch
        (iago_play_endgame) plays them all out (launches = 2); the turn loop solves per turn: the same records.
        explore_turns = e (an int >= 0; None or 0, the default: off): at a searched turn t < e (the game's turn counter,
        passes included) the move is not the most visited child but drawn in proportion to the root's visit counts
        (temperature 1), so that the games of a batch leave the opening on different lines.  The draw is in integers
        (include/iago_hip_serving.h, iago_mcts_search_explore): with n the turn's visit row `pi`, N its sum and w the
        Philox word of (seed ^ EXPLORE_SEED_XOR; game_id_base + g, t), the lowest cell a with sum_{b <= a} n[b] >
        (w * N) >> 32.  The record keeps its shape (valid 1, pi the visit row, move the drawn move); the one launch and
        the turn loop play the same games; solve_empties composes (a parked turn is not searched, so not drawn).
        playout_cap = (n_fast, full_per_256) (None, the default: off): playout-cap randomisation.  Every searched turn
        t of game g is FULL -- n_sims playouts, valid 1, a policy target -- when the top byte of the Philox word of
        (seed ^ CAP_SEED_XOR; game_id_base + g, t) is below full_per_256 (1 .. 256), else FAST: the first n_fast (1 ..
        n_sims) playouts of the same search, the move played as ever (the most visited child; below explore_turns the
        draw), recorded with valid 4 and its visit row, kept out of tuples() and given by fast_tuples().  sim_counter
        advances by n_sims per turn all the same.  The one launch (iago_mcts_search_cap) and the turn loop play the same
        games; solve_empties and explore_turns compose.
        root_noise = (alpha_256, eps_256[, draws]) (None, the default: off): Dirichlet-style noise on the root's priors,
        in integers (include/iago_hip_serving.h, iago_mcts_root_noise).  At every searched turn t of game g with K >= 2
        legal moves a Polya urn -- every legal cell starts with mass alpha = alpha_256 / 256 (1 .. 4096), `draws` draws N
        (a power of two in 16 .. 1024, default 256) each in proportion to alpha + the cell's count so far, Philox words
        of (seed ^ NOISE_SEED_XOR; game_id_base + g, t, j >> 2) -- gives counts c that are Dirichlet-multinomial(N,
        alpha), and the stored prior p of the root's child a becomes p (256 - eps_256) / 256 + eps_256 c[a] / (256 N)
        (eps_256 0 .. 256), two float32 roundings, for the whole of the turn's search.  Under playout_cap only the FULL
        turns are noised (a fast turn searches the clean priors, so it is no longer a prefix of the full turn's search).
        The records keep their shape.  Such games ALWAYS run through the turn loop (launches = their turns; per turn
        iago_mcts_root_noise, then iago_mcts_search_noise, on the role split where the engine has it), and play_stream
        through the batch loop; solve_empties, explore_turns and playout_cap compose; eps_256 = 0 plays the games of
        root_noise=None.
        forced_playouts = k_256 (None, the default: off; an int in 1 .. 4096, k = k_256 / 256, KataGo's k = 2 is 512;
        only with root_noise, else ValueError -- root_noise=(alpha_256, 0) forces without mixing): KataGo's forced playouts
        and policy-target pruning (include/iago_hip_serving.h, iago_mcts_search_forced / iago_mcts_prune_visits).  In every
        noised search a child of the ROOT with n >= 1 visits and stored (mixed) prior p is taken before any other while
        256 n^2 < k_256 p N, N the root's visits; after the search every child but the most visited one gives back up to
        as many visits as were forced, one at a time while its PUCT score stays below the most visited child's, and a
        child left with one visit gives that back too.  The move is chosen from the RAW counts as ever; `pi` records the
        PRUNED row and the new record `pi_raw` the raw one (tuples() hand the trainer the pruned targets).  Under
        playout_cap only the FULL turns are forced and pruned: a fast row's pi is its raw row.  Without forced playouts
        the result's pi_raw is None.
        solved_targets = True (False, the default: off; only with solve_empties, else ValueError): every solved turn also
        records the SET of its optimal moves in `best` ((T, B) int64: bit a set iff move a reaches the turn's exact
        score; 0 on every row that is not solved) -- the turn loop through ops.solve_endgame_moves(moves="best"), the
        play-out launch through iago_play_endgame_moves: the same records, and every other record as without it.
        solved_tuples() then carries best and a 0 / 1 `pi`, a noise-free policy target for the plies the search never
        sees.  Without it the result's best is None.
        gumbel = (m, c_scale_256[, c_visit]) (None, the default: off -- the engine of before, argument for argument; m in 2
        .. 64, c_scale_256 in 1 .. 4096, c_visit in 0 .. 4096, default 50): the Gumbel root search of Danihelka et al. 2022
        (include/iago_hip_serving.h, iago_mcts_search_gumbel), for engines with backup="negamax" and selection="alphazero".
        Every searched turn starts from a FRESH root (no subtree reuse), draws one Gumbel per cell from (seed ^
        GUMBEL_SEED_XOR; game_id_base + g, t, cell), spends the n_sims playouts on the top min(m, K) moves by g + logit
        in sequential halving, and plays the survivor: the best of the most visited moves by g + logit + sigma(q).  `pi`
        records the improved policy round(65536 softmax(logit + sigma(completed q))) (gumbel_targets) and `pi_raw` the
        visit row; `move` is the survivor.  Such games ALWAYS run through the turn loop.  solve_empties and playout_cap
        compose (under a cap only the FULL turns run the rule: a fast turn is the plain search's, pi = pi_raw);
        explore_turns, root_noise and forced_playouts are refused beside it -- the rule explores by its own draw.
        root_values = True (False, the default: off; for engines with backup="negamax", else ValueError): every searched
        turn also records its root's value from the MOVER's view in Q16 in `q` ((T, B) int32: rint(-root.q * 65536) read
        after the search and before the tree moves on, BatchedMCTS.root_value; 0 on every row whose valid is not 1 or 4)
        and the root's visits in `q_visits` -- what SelfPlayResult.value_targets and tuples(value_target=) turn into the
        Value net's targets.  Such games ALWAYS run through the turn loop (the whole-game launch does not record root
        values), with one more small launch per side and turn and still ONE readback per turn; the record changes no game:
        every other record and every move are those of root_values=False.  Every other rule composes.  Without it the
        result's q and q_visits are None."""
        return self._play(n_sims, handicap, record,
                          _play_rules(n_sims, solve_empties, explore_turns, playout_cap, root_noise, forced_playouts,
                                      solved_targets, gumbel, root_values))

    def _play(self, n_sims, handicap, record, rules):
        """play() under validated rules (a PlayRules)."""
        self.mcts._backup_check(rules)   # (an engine the rules are not offered for: refused before anything is reset)
        res = self._one_launch(n_sims, self.B, handicap, record, rules)
        if res is None:
            res = self._play_turns([_Side(self.mcts, n_sims)], *self._start_boards(self.B, handicap), record,
                                   SelfPlayResult(), rules)
        return res

    def play_stream(self, n_sims, n_games, handicap=None, record=True, solve_empties=None, explore_turns=None,
                    playout_cap=None, root_noise=None, forced_playouts=None, solved_targets=False, gumbel=None,
                    root_values=False):
        """n_games self-play games, at most B (the engine's slots) of them in play at a time, as ONE persistent launch
        where play() applies: a slot whose game ends takes the next game id on the device and plays that game from its
        first turn (iago_mcts_search_args.games_total), so the launch ends once, with the last game, instead of every B
        games.  Game G is bit for bit game G of the BATCH LOOP -- play() ceil(n_games / B) times, batch k with
        game_id_base + k B, each from the same sim_counter -- which is also the path taken where the one launch does not
        apply (another engine, pools that cannot hold a whole game, z_log or trace; and, as a replay, a pool that filled
        up in the launch).  handicap: (n_games,) int64 bit masks of extra colour-2 stones.  The result has n_games
        columns (tuples() give the game ids game_id_base ..); n_turns is the longest game's, `launches` the launches it
        took (1: the stream); sim_counter ends n_turns x n_sims on, as after one batch.  solve_empties: as in play() --
        the stream's games hand over at k empties and one launch plays all n_games out (launches = 2).  explore_turns:
        as in play() -- game G draws with its own id, whichever slot plays it.  playout_cap: as in play() -- game G's
        turns are full or fast by its own id.  root_noise: as in play() -- game G's urns are keyed by its own id.
        forced_playouts: as in play(), with the record pi_raw.  solved_targets: as in play(), with the record best.
        gumbel: as in play() -- the batch loop, game G's draws keyed by its own id, with the record pi_raw.
        root_values: as in play() -- the batch loop, with the records q and q_visits."""
        rules = _play_rules(n_sims, solve_empties, explore_turns, playout_cap, root_noise, forced_playouts, solved_targets,
                            gumbel, root_values)
        m, T = self.mcts, self.max_turns
        m._backup_check(rules)
        n_games = int(n_games)
        if n_games < 1:
            raise ValueError("play_stream: n_games >= 1 expected")
        if n_games * T * 64 * 4 > STREAM_REC_BYTES:
            raise ValueError("play_stream: %d games x %d turns of visit counts exceed %d bytes: fewer games per call"
                             % (n_games, T, STREAM_REC_BYTES))
        if handicap is not None and tuple(handicap.shape) != (n_games,):
            raise ValueError("play_stream: handicap is an (n_games,) int64 tensor")
        plain = getattr(m, "z_log", None) is None and getattr(m, "trace", None) is None
        res = self._one_launch(n_sims, n_games, handicap, record, rules, applies=plain, games_total=n_games)
        if res is None:
            res = self._play_batches(n_sims, n_games, handicap, record, rules)
        return res

    def play_match(self, n_sims, mcts_colour=None, record=True, solve_empties=None, forced_playouts=None, opponent=None,
                   opening_turns=0, paired=False, gumbel=None):
        """B games of PV-MCTS (n_sims playouts per move) against the SL policy it is built on -- the reference's
        `game.py --auto` (game.py:96-145,246-262) -- with the engine's nets: in game g PV-MCTS plays colour
        mcts_colour[g] (1 moves first; an int: every game; 2, the default, is the reference's setting) and the policy
        net (the engine's policy_fn) the other colour.  PV-MCTS searches from its tree as in play(); the policy's move is
        the masked draw of ops.sample_moves from the net's distribution of the position, with the uniform of
        (seed ^ MATCH_SEED_XOR, game_id_base + g, turn, stream 0), and advances the tree like any move (game.py:107); a
        final move that is the only one (stone_num > 62) is played by either side without a search and without
        update_with_move (game.py:97-98).  ONE launch of the persistent search where play() takes it, else (and when a
        pool fills up in the launch) the turn loop: the same games record for record.  sim_counter advances by
        n_sims per turn, searched or not.  Returns a MatchResult.  solve_empties = k (as in play()): PV-MCTS plays the
        exact solver's move at its turns of at most k empties (valid 3) -- not the forced final move, which keeps
        precedence (valid 2), and not the policy's turns.  Such a match ALWAYS runs through the turn loop (launches =
        its turns): a one-launch match cannot hand its games over, the policy side needs the net workgroups to the last
        move.  forced_playouts: None; anything else is a ValueError (a match has no root noise and does not force).
        opponent = AlphaBeta(d) (None, the default: the policy net): the other colour's moves are the fixed-depth
        alpha-beta search's (ops.alphabeta_moves at depth d: the lowest-indexed move of the best value), an opponent that
        owes nothing to the nets.  Its move is recorded with valid 2 and advances the tree like any move; the only final
        move keeps its precedence; solve_empties still applies to PV-MCTS's turns alone; a position the opponent does not
        finish raises IagoError.  AlphaBeta(d, split=1 or 2) plays the same moves from ops.alphabeta_moves(split=), every
        root's search spread over the lanes, with room for B x ALPHABETA_JOBS_PER_ROOT[split] jobs per turn and still one
        readback per turn: a turn whose jobs do not fit takes the unsplit launch's moves and is counted in the result's
        split_overflows.  opening_turns = e (an even int in [0, 16]; 0, the default: none): at the turns below e
        nobody searches and both colours play ops.random_moves' move -- the r-th lowest legal cell, r = (w * K) >> 32 with
        w the Philox word of (seed ^ OPENING_SEED_XOR; game_id_base + g mod id_mod, t) -- recorded with valid 5
        (REC_OPENING: tuples() never see them), so that a batch against a deterministic opponent is many games.
        ("Nobody searches": no game is in the search's mask.  The turn loop still launches the search with an empty mask
        at an opening turn, as it does at the opponent's turns, which keeps sim_counter advancing by n_sims per turn.)
        paired = True (needs an even B, and no mcts_colour: it sets it): games g and g + B / 2 draw the same opening
        (id_mod = B / 2, else B) and PV-MCTS plays colour 1 in the first half and colour 2 in the second.  With an
        opponent or opening_turns > 0 the match ALWAYS runs through the turn loop (launches = its turns); with all three at
        their defaults it is the match above, argument for argument.  mcts_colour: None is 2, or with paired the halves.
        gumbel = (m, c_scale_256[, c_visit]) (None, the default: off): PV-MCTS's searched turns run the Gumbel root search
        as in play() -- fresh roots, the survivor for a move, pi the improved policy and pi_raw the visit row.  Such a
        match ALWAYS runs through the turn loop."""
        _no_forced_playouts(forced_playouts, "play_match")
        rules = _play_rules(n_sims, solve_empties, gumbel=gumbel)
        match = _match_rules(opponent, opening_turns, paired, mcts_colour, self.B)
        dev = self.mcts.cur_own.device
        if paired:
            col = torch.cat([torch.full((self.B // 2,), c, dtype=torch.int8, device=dev) for c in (1, 2)])
        else:
            col = _colour_arg(2 if mcts_colour is None else mcts_colour, self.B, dev, "play_match: mcts_colour")
        self.mcts._backup_check(rules)   # (a hooked negamax engine, say: refused before anything is reset)
        codes = torch.where(col == 1, _lib.MATCH_MCTS_COLOUR_1, _lib.MATCH_MCTS_COLOUR_2).to(torch.uint8)
        plain = match.opponent is None and match.opening_turns == 0
        res = self._one_launch(n_sims, self.B, None, record, rules, applies=rules.solve_empties is None and plain,
                               active=codes, res=MatchResult())
        if res is None:
            res = self._play_turns([_Side(self.mcts, n_sims, col)], *self._start_boards(self.B), record, MatchResult(),
                                   rules, policy_moves=True, match=None if plain else match)
        res.mcts_colour = col
        return res

    def _play_batches(self, n_sims, n_games, handicap, record, rules):
        """play_stream's batch loop: ceil(n_games / B) batches of play() under `rules`, batch k with game_id_base + k B
        and the same sim_counter, the first n_games columns kept."""
        m, B = self.mcts, self.B
        base, s0 = m.game_id_base, m.sim_counter
        parts = []
        try:
            for k in range(-(-n_games // B)):
                w = min(B, n_games - k * B)
                hc = None
                if handicap is not None:
                    hc = torch.zeros(B, dtype=torch.int64, device=handicap.device)
                    hc[:w] = handicap[k * B:k * B + w]
                m.game_id_base, m.sim_counter = base + k * B, s0
                parts.append((self._play(n_sims, hc, record, rules), w))
        finally:
            m.game_id_base = base
        res = SelfPlayResult()
        # (a batch played through the turn loop has no per-game end turns: its records give them)
        turns = [r.game_turns if r.game_turns is not None or not record else _end_turns(r.valid) for r, _ in parts]
        if any(x is None for x in turns):
            res.game_turns = None
            t = max(r.n_turns for r, _ in parts)
        else:                                  # (the longest of the games kept, as in the one launch)
            res.game_turns = torch.cat([x[:w] for x, (_, w) in zip(turns, parts)])
            t = int(res.game_turns.max().item())
        m.sim_counter = (s0 + t * n_sims) & 0xFFFFFFFF
        res.game_id_base, res.n_turns, res.launches = base, t, len(parts)
        res.mover = [1 if k % 2 == 0 else 2 for k in range(t)]
        res.z = torch.cat([r.z[:w] for r, w in parts])
        res.final_p1 = torch.cat([r.final_p1[:w] for r, w in parts])
        res.final_p2 = torch.cat([r.final_p2[:w] for r, w in parts])
        if record:
            cols = {k: [] for k in ("own", "opp", "valid", "move", "pi", "score")}
            if RootRule.of(rules) is not None and RootRule.of(rules).targets:
                cols["pi_raw"] = []
            if rules.solved_targets:
                cols["best"] = []
            if rules.root_values:
                cols["q"], cols["q_visits"] = [], []
            for r, w in parts:
                dev, rows = r.z.device, min(r.n_turns, t)
                pad = t - rows
                # (rows past a batch's last turn: what the one launch records after a game's end -- the final
                # boards still swapping sides, no move)
                tw = (torch.arange(rows, t, device=dev) % 2 == 0).reshape(pad, 1)
                p1, p2 = r.final_p1[:w].reshape(1, w), r.final_p2[:w].reshape(1, w)
                cols["own"].append(torch.cat([r.own[:rows, :w], torch.where(tw, p1, p2)]))
                cols["opp"].append(torch.cat([r.opp[:rows, :w], torch.where(tw, p2, p1)]))
                cols["valid"].append(torch.cat([r.valid[:rows, :w], r.valid.new_zeros((pad, w))]))
                cols["move"].append(torch.cat([r.move[:rows, :w], r.move.new_full((pad, w), -1)]))
                cols["pi"].append(torch.cat([r.pi[:rows, :w], r.pi.new_zeros((pad, w, 64))]))
                if "pi_raw" in cols:
                    cols["pi_raw"].append(torch.cat([r.pi_raw[:rows, :w], r.pi_raw.new_zeros((pad, w, 64))]))
                if "best" in cols:
                    cols["best"].append(torch.cat([r.best[:rows, :w], r.best.new_zeros((pad, w))]))
                for name in ("q", "q_visits") if "q" in cols else ():
                    cols[name].append(torch.cat([getattr(r, name)[:rows, :w], r.q.new_zeros((pad, w))]))
                cols["score"].append(torch.cat([r.score[:rows, :w], r.score.new_zeros((pad, w))]))
            for k, v in cols.items():
                setattr(res, k, torch.cat(v, dim=1))
        return res


class ArenaResult(SelfPlayResult):
    """The games of ArenaEngine.play: PV-MCTS with agent A's nets against PV-MCTS with agent B's.  As a SelfPlayResult
    (valid 1 where the mover searched, 0 for a pass or no turn; pi the MOVER's visit row), with agent: (T, B) uint8, whose
    turn it was (0 = A, 1 = B: the colour rule, searched or not), and a_colour: (B,) int8, the colour A played in each
    game."""

    SCORE_RECORD = None   # (no solver in the arena: no `score` record)

    def score(self):
        """A's results: dict(wins, draws, losses, n, win_rate), a draw counting 1/2 (MatchResult.score's arithmetic)."""
        z = self.z.to(torch.int32) * torch.where(self.a_colour == 1, 1, -1).to(torch.int32)
        wins, draws, losses = (int(v) for v in torch.stack([(z > 0).sum(), (z == 0).sum(), (z < 0).sum()]).tolist())
        n = wins + draws + losses
        return dict(wins=wins, draws=draws, losses=losses, n=n, win_rate=(wins + 0.5 * draws) / n if n else float("nan"))

    def tuples(self, agent=None):
        """SelfPlayResult.tuples() -- the searched rows, in the shape ReinforceTrainer.add_to_window takes -- of both
        agents (None) or of the rows agent 0 (A) / 1 (B) searched only."""
        if agent is None:
            return SelfPlayResult.tuples(self)
        if isinstance(agent, bool) or agent not in (0, 1):
            raise ValueError("tuples: agent is None, 0 (A) or 1 (B), not %r" % (agent,))
        full = self.valid
        try:
            self.valid = ((full == 1) & (self.agent == agent)).to(full.dtype)
            return SelfPlayResult.tuples(self)
        finally:
            self.valid = full


class ArenaEngine(object):
    """Whole games between TWO PV-MCTS agents, each with its own nets and search constants: mcts_a and mcts_b, two
    BatchedMCTS on the persistent search (wave == 1) with equal n_games and device and separate tree pools.  What
    SelfPlayEngine.play_match cannot say -- whether this round's prior, value net and lmbda together beat last round's,
    100 playouts against 400, lmbda 0.5 against 0 -- is ArenaResult.score().

    The two engines should differ in `game_id_base` or `seed`: otherwise game g's rollouts draw the SAME Philox stream on
    both sides (the streams are keyed by seed, game id and playout count, and both engines count their playouts alike).

    The games run through SelfPlayEngine._play_turns with two sides of complementary colours (every mover with a legal
    move searches, no forced final move): the turn loop is self-play's, the one difference is who searches.  At turn t
    the mover of game g is A iff a_colour[g] == (1 if t % 2 == 0 else 2); A searches its movers from its tree, B its
    movers from its tree, the move is the mover's best_move (below explore_turns: its draw_move, keyed by that engine's
    own seed and id), and BOTH trees advance by every move.  One ops.play_turn and one host readback per turn.  The
    turn's searches are this class's (_search_both), in two forms, the same games record for record: sequential
    (mcts_a.search, then mcts_b.search) and one launch per turn (iago_mcts_search_arena: both searches in one grid);
    either way both engines' sim_counter advance by their n_sims every turn, whoever had movers.

    Not here: whole arena games in one launch (a game's two trees live in different workgroups), the role split and more
    games per agent than a single launch holds, solve_empties, streams, more than two agents, an Elo table."""

    # play(one_launch=None): the form that measured faster at 1024 games x 100 playouts (LABNOTES.md, "Arena")
    ONE_LAUNCH_DEFAULT = False

    def __init__(self, mcts_a, mcts_b, max_turns=_lib.IAGO_MAX_TURNS):
        for name, m in (("mcts_a", mcts_a), ("mcts_b", mcts_b)):
            if not getattr(m, "persistent", False):
                raise ValueError("%s must be a BatchedMCTS on the persistent search" % name)
            if getattr(m, "wave", 1) != 1 or getattr(m, "wave_entry", False):
                raise ValueError("%s must have wave == 1 (the arena searches one playout per tree at a time)" % name)
        if mcts_b is mcts_a or mcts_b.tree is mcts_a.tree:
            raise ValueError("mcts_b must have a tree pool of its own (two engines, two pools)")
        if mcts_b.n_games != mcts_a.n_games:
            raise ValueError("mcts_b must have mcts_a's n_games (%d, not %d)" % (mcts_a.n_games, mcts_b.n_games))
        if mcts_b.cur_own.device != mcts_a.cur_own.device:
            raise ValueError("mcts_b must be on mcts_a's device (%s, not %s)" % (mcts_a.cur_own.device, mcts_b.cur_own.device))
        if isinstance(max_turns, bool) or not isinstance(max_turns, numbers.Integral) or not 1 <= max_turns <= _lib.IAGO_MAX_TURNS:
            raise ValueError("max_turns must be an int in [1, %d], not %r" % (_lib.IAGO_MAX_TURNS, max_turns))
        self.a, self.b = mcts_a, mcts_b
        self.B = mcts_a.n_games
        self.max_turns = int(max_turns)
        self.device = mcts_a.cur_own.device
        self.net_workgroups = None   # of the one launch (None: not sized yet; 0: it does not fit this device)
        self.n_arena_launches = 0

    def _colours(self, a_colour):
        """play's a_colour as a (B,) int8 tensor of 1 / 2 (validated as play_match's mcts_colour is).  None: A plays
        colour 1 in the games [0, B/2) and colour 2 in the rest -- blocks, not alternation, so that at every turn each
        agent's movers fill whole game workgroups (a workgroup without a mover finishes at once and serves nets)."""
        B, dev = self.B, self.device
        if a_colour is None:
            col = torch.full((B,), 2, dtype=torch.int8, device=dev)
            col[:B // 2] = 1
            return col
        return _colour_arg(a_colour, B, dev, "play: a_colour", "None, ")

    @staticmethod
    def _n_sims(n_sims):
        """play's n_sims: an int >= 1 for both agents, or a pair (n_a, n_b) of them."""
        pair = tuple(n_sims) if isinstance(n_sims, (tuple, list)) else (n_sims, n_sims)
        if len(pair) != 2 or any(isinstance(n, bool) or not isinstance(n, numbers.Integral) or n < 1 for n in pair):
            raise ValueError("play: n_sims is an int >= 1 or a pair (n_a, n_b) of them, not %r" % (n_sims,))
        return int(pair[0]), int(pair[1])

    def _size_launch(self):
        """The one launch's net workgroups (0: both agents' game workgroups and two net workgroups do not fit), and each
        engine's rows of wg_own / wg_opp for them: any workgroup of the arena's grid may walk either agent's nets."""
        a, b = self.a, self.b
        resident = min(a.resident_workgroups, b.resident_workgroups)
        games = sum(-(-m.n_games // m.games_per_workgroup) for m in (a, b))
        net = min(max(a.net_workgroups, b.net_workgroups, 2), resident - games)
        self.net_workgroups = net if net >= 2 else 0
        if self.net_workgroups:
            for m in (a, b):
                m.reserve_net_rows(games + self.net_workgroups)

    def _search_both(self, sides, own, opp, one_launch):
        """The turn's searches for the turn loop: A's movers (sides[0].act) from A's tree, B's (sides[1].act) from B's,
        each side's `counts` being [its games searched, the nodes of its fullest pool].  Returns the launches it took."""
        a, b = self.a, self.b
        (s_a, n_a, c_a), (s_b, n_b, c_b) = ((s.act, s.n_sims, [int(v) for v in s.counts]) for s in sides)
        if one_launch and self.net_workgroups is None:
            self._size_launch()
        # (a turn at which one agent has no mover is ONE launch anyway: today's)
        if one_launch and self.net_workgroups and c_a[0] and c_b[0]:
            for m, c in ((a, c_a), (b, c_b)):
                m._forget_stale_values()
                m._fresh_count.zero_()
                m._compact_if_half_full(c[1])
            args_a, keep_a = a._search_args(own, opp, s_a, n_a)
            args_b, keep_b = b._search_args(own, opp, s_b, n_b)
            args_a.net_workgroups = args_b.net_workgroups = self.net_workgroups
            rc = ops.search_arena(args_a, args_b, check_result=False)
            if rc == _lib.IAGO_OK:
                a._ps_keep, b._ps_keep = keep_a + (None,), keep_b + (None,)   # alive until the next launch
                for m, c, n in ((a, c_a, n_a), (b, c_b, n_b)):
                    m.sim_counter = (m.sim_counter + n) & 0xFFFFFFFF
                    m.n_leaf_evals += c[0] * n
                self.n_arena_launches += 1
                return 1
            if rc != _lib.IAGO_ERR_CAPACITY:
                check(rc, "iago_mcts_search_arena")
            self.net_workgroups = 0   # (nothing was launched: the sequential form from here on)
        a.search(own, opp, s_a, n_a, counts=c_a, check=False)   # (sim_counter: + n_sims whoever searched)
        b.search(own, opp, s_b, n_b, counts=c_b, check=False)
        return (1 if c_a[0] else 0) + (1 if c_b[0] else 0)

    def play(self, n_sims, a_colour=None, record=True, explore_turns=None, one_launch=None, forced_playouts=None,
             gumbel=None):
        """B games from the opening, both trees fresh.  n_sims: playouts per move, an int or a pair (n_a, n_b); a_colour:
        the colour A plays, 1, 2 or a (B,) integer tensor of 1 / 2 (None: 1 in the first half of the games, 2 in the
        rest); explore_turns: as SelfPlayEngine.play's, each mover drawing with its own engine's seed and id; one_launch:
        True = one iago_mcts_search_arena launch per turn (the sequential form where the library answers
        IAGO_ERR_CAPACITY), False = the sequential form, None = ONE_LAUNCH_DEFAULT.  forced_playouts: None; anything else
        is a ValueError (the arena has no root noise and does not force).  gumbel: None; anything else is a ValueError
        (two searches in one launch do not take the Gumbel root search).  Returns an ArenaResult."""
        _no_forced_playouts(forced_playouts, "ArenaEngine.play")
        if gumbel is not None:
            raise ValueError("ArenaEngine.play: gumbel is not available (the Gumbel root search lives in the turn loop of "
                             "play / play_stream / play_match)")
        n_a, n_b = self._n_sims(n_sims)
        col = self._colours(a_colour)
        rules = _play_rules(n_a, explore_turns=explore_turns)
        if one_launch is not None and not isinstance(one_launch, bool):
            raise ValueError("play: one_launch is None, True or False, not %r" % (one_launch,))
        one = self.ONE_LAUNCH_DEFAULT if one_launch is None else one_launch
        for m in (self.a, self.b):   # (a hooked negamax engine: refused before anything is reset)
            BatchedMCTS._backup_check(m)
        self.a.tree.reset()
        self.b.tree.reset()
        loop = SelfPlayEngine(self.a, self.max_turns)
        res = loop._play_turns([_Side(self.a, n_a, col), _Side(self.b, n_b, 3 - col)], *loop._start_boards(self.B), record,
                               ArenaResult(), rules,
                               search=lambda sides, own, opp, rules: self._search_both(sides, own, opp, one))
        res.a_colour = col
        if record:
            # (whose turn it was is the colour rule, searched or not: A's where the turn's mover has A's colour)
            mover = torch.tensor(res.mover, dtype=torch.int8, device=self.device).reshape(-1, 1)
            res.agent = (col.reshape(1, self.B) != mover).to(torch.uint8)
        return res


def _most_empties(own, opp):
    """The stack the solver needs: the most empties of the positions, capped at what it takes (beyond: refused)."""
    bits = ops.tensor_to_bits(own | opp)
    return min(max((64 - bin(int(b)).count("1") for b in bits), default=0), _lib.ENDGAME_MAX_EMPTIES)


def solve_endgame(own, opp, mode="exact", split_depth=0, time_limit_ms=ops.ENDGAME_TIME_LIMIT_MS):
    """ops.solve_endgame for one position or a few, with a root split: every position is expanded `split_depth` plies
    (a pass is a ply; a finished game is not expanded) with ops.legal_moves / ops.apply_moves, all the leaves are
    solved in ONE launch with the full window, and the values are minimaxed back, the lowest-indexed move winning ties.
    The result equals split_depth = 0's (score and move); what it buys is lanes: a single position at 14+ empties
    spreads over the chip instead of running on one lane.  Returns the dict of ops.solve_endgame for the roots (nodes:
    the leaves' nodes plus the split's own; ctl: the launch's)."""
    if not isinstance(split_depth, int) or isinstance(split_depth, bool) or split_depth < 0:
        raise ValueError("split_depth must be an int >= 0, got %r" % (split_depth,))
    dev = own.device
    if split_depth == 0:
        return ops.solve_endgame(own, opp, mode=mode, max_empties=_most_empties(own, opp), time_limit_ms=time_limit_ms)
    n = own.numel()
    # levels[k]: (own, opp) device tensors of the nodes at ply k, their parent at ply k - 1 and the move from it
    nodes = [(own.reshape(n).contiguous(), opp.reshape(n).contiguous(), None, None)]
    leaf = []   # per level: bool numpy array, the node is solved by the kernel
    for depth in range(split_depth + 1):
        o, p, _, _ = nodes[depth]
        m = o.numel()
        legal = ops.tensor_to_bits(ops.legal_moves(o, p))
        other = ops.tensor_to_bits(ops.legal_moves(p, o))
        over = (legal == 0) & (other == 0)
        if depth == split_depth:
            leaf.append(np.ones(m, bool))
            break
        leaf.append(over.copy())
        parent, move = [], []
        for i in range(m):
            if over[i]:
                continue
            lm = int(legal[i])
            if lm == 0:
                parent.append(i)
                move.append(-1)   # the pass child
            while lm:
                b = lm & -lm
                parent.append(i)
                move.append(b.bit_length() - 1)
                lm ^= b
        idx = torch.tensor(parent, dtype=torch.int64, device=dev)
        mv = torch.tensor(move, dtype=torch.int8, device=dev)
        co, cp = o[idx].contiguous(), p[idx].contiguous()
        ops.apply_moves(co, cp, mv)
        nodes.append((cp, co, np.array(parent, np.int64), np.array(move, np.int64)))   # the other side moves next
    # every leaf in one launch
    lo = torch.cat([nodes[k][0][torch.from_numpy(np.nonzero(leaf[k])[0]).to(dev)] for k in range(len(leaf))])
    lp = torch.cat([nodes[k][1][torch.from_numpy(np.nonzero(leaf[k])[0]).to(dev)] for k in range(len(leaf))])
    lo, lp = lo.contiguous(), lp.contiguous()
    res = ops.solve_endgame(lo, lp, mode=mode, max_empties=_most_empties(lo, lp), time_limit_ms=time_limit_ms)
    score_l, move_l = res["score"].cpu().numpy().astype(np.int64), res["move"].cpu().numpy().astype(np.int64)
    nodes_l = res["nodes"].cpu().numpy()
    # minimax back, deepest level first: value = max over children of -child, the first (lowest-index) maximum wins
    val, mov, cnt, at = [], [], [], 0
    for k in range(len(leaf)):
        m = len(leaf[k])
        val.append(np.zeros(m, np.int64))
        mov.append(np.full(m, -3, np.int64))
        cnt.append(np.ones(m, np.int64))
        sel = np.nonzero(leaf[k])[0]
        val[k][sel] = score_l[at:at + len(sel)]
        mov[k][sel] = move_l[at:at + len(sel)]
        cnt[k][sel] = nodes_l[at:at + len(sel)]
        at += len(sel)
    for k in range(len(leaf) - 1, 0, -1):
        parent, move = nodes[k][2], nodes[k][3]
        best = np.full(len(leaf[k - 1]), -1000, np.int64)
        for j in range(len(parent)):   # children in ascending move order per parent (-1, the pass, is alone)
            i = parent[j]
            cnt[k - 1][i] += cnt[k][j]
            if -val[k][j] > best[i]:
                best[i] = -val[k][j]
                mov[k - 1][i] = move[j]
        inner = ~leaf[k - 1]
        val[k - 1][inner] = best[inner]
    return dict(score=torch.from_numpy(val[0].astype(np.int8)).to(dev), move=torch.from_numpy(mov[0].astype(np.int8)).to(dev),
                nodes=torch.from_numpy(cnt[0]).to(dev), solved=torch.ones(n, dtype=torch.uint8, device=dev),
                ctl=res["ctl"])


def endgame_errors(own, opp, move, max_empties=_lib.ENDGAME_MAX_EMPTIES, mode="exact", time_limit_ms=ops.ENDGAME_TIME_LIMIT_MS,
                   split=0):
    """The loss against perfect play of moves actually played: how many discs (mode "wld": outcomes) each move gives
    away.  own / opp: (n,) int64 positions, own = the mover; move: (n,) integer tensor, the move played there.  Rows
    with move < 0 (a pass, no turn) or more than max_empties empties are skipped and counted; the others are solved in
    ONE launch of ops.solve_endgame_moves(moves="all"), which knows the exact value of every move.  Returns a dict: as
    device tensors over the rows kept, in their order, index (their row numbers in the input), score (the position's
    value), played (the value of the move played), loss = score - played (>= 0), optimal (loss == 0) and blunder (the
    sign of the value changed: a win given away, or a draw turned into a loss); as Python numbers rows, skipped,
    mean_loss, optimal_rate and blunder_rate (nan without rows).  A move that is not legal is a ValueError naming the
    row; a position the solver refuses (own & opp != 0) raises ops.solve_endgame_moves' IagoError.  split (0, 1 or
    2) goes to ops.solve_endgame_moves: the same answers with every root spread over the lanes."""
    n = own.numel()
    if opp.numel() != n or move.numel() != n:
        raise ValueError("endgame_errors: own / opp / move sizes differ")
    k = _solve_empties_arg(max_empties)
    if k is None:
        raise ValueError("endgame_errors: max_empties must be an int in [0, %d]" % _lib.ENDGAME_MAX_EMPTIES)
    own, opp, move = own.reshape(n), opp.reshape(n), move.reshape(n).to(torch.int64)
    keep = (move >= 0) & (_empties(own, opp) <= k)
    index = torch.nonzero(keep).reshape(-1)
    r = ops.solve_endgame_moves(own[index].contiguous(), opp[index].contiguous(), mode=mode, moves="all", max_empties=k,
                                time_limit_ms=time_limit_ms, split=split)
    mv = move[index]
    played = r["move_score"].to(torch.int32).gather(1, mv.clamp(max=63).reshape(-1, 1)).reshape(-1)
    illegal = (played == _lib.ENDGAME_NO_MOVE) | (mv > 63)
    score = r["score"].to(torch.int32)
    loss = score - played
    optimal, blunder = loss == 0, torch.sign(played) != torch.sign(score)
    legal = ~illegal
    rows = int(index.numel())
    back = _read_back(dict(illegal=illegal.any(), first=index[illegal.to(torch.int64).argmax()] if rows else None,
                           loss=(loss * legal).sum(), optimal=(optimal & legal).sum(), blunder=(blunder & legal).sum()))
    if back["illegal"]:
        i = back["first"]
        raise ValueError("endgame_errors: row %d: move %d is not a legal move of the side to move" % (i, int(move[i].item())))
    rate = (lambda v: v / rows) if rows else (lambda v: float("nan"))
    return dict(index=index, score=score, played=played, loss=loss, optimal=optimal, blunder=blunder, rows=rows,
                skipped=n - rows, mean_loss=rate(back["loss"]), optimal_rate=rate(back["optimal"]),
                blunder_rate=rate(back["blunder"]))
