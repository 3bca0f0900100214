"""The refusals of the persistent search's host launch layer (csrc/search_kernel.hip, from iago_mcts_search_capacity
on), without a GPU: every case starts from a valid argument set for its entry point, breaks ONE thing, calls the entry
point and pins the exact return code and the exact iago_last_error() text -- so that whoever reorders that layer sees
which check was lost.  One case per refusal that is reached before the first question to the device, and for the two
large null-or-misaligned conditions one case per pointer and per alignment clause.

Nothing here can be launched, on any machine: the argument structs are real host structs, but every device pointer is
a made-up aligned constant, and every base set has value->n = policy->n = 0, which the nets'-rows check refuses after
the device queries and before anything is zeroed or launched (without a device the first query refuses it).
`active` is a real host array: the park / explore / cap / arena checks read it."""
import ctypes as C

import pytest

from iago_amd import _lib

OK, INVALID, HIP, CAPACITY = _lib.IAGO_OK, _lib.IAGO_ERR_INVALID, _lib.IAGO_ERR_HIP, _lib.IAGO_ERR_CAPACITY

FAKE = 0x7E0000000000   # never dereferenced: the refusals under test come before any use of it


def _fake(k, who=0):
    """A made-up device pointer, 4096-byte aligned, distinct per (k, who)."""
    return FAKE + who * 0x10000000 + k * 0x1000


class Call(object):
    """A valid call of one entry point: the argument structs and what they point to (kept alive here)."""

    def __init__(self, entry, whole=False, n_games=4, width=1, who=0, park=False):
        self.entry, self.width = entry, width
        p = iter(range(1, 64))
        f = lambda: _fake(next(p), who)
        t = self.tree = _lib.MctsTree()
        t.n_games, t.capacity, t.has_v = n_games, 1024, 1
        t.nodes, t.n_nodes, t.root, t.overflow = f(), f(), f(), f()
        self.active = (C.c_uint8 * n_games)(*([1] * n_games))
        a = self.a = _lib.MctsSearchArgs()
        a.tree = C.addressof(t)
        a.root_own, a.root_opp = f(), f()
        a.active = C.addressof(self.active)
        a.c_puct, a.lmbda, a.n_thr, a.n_sims, a.net_workgroups = 1.0, 0.5, 15, 16, 16
        a.cur_node, a.cur_own, a.cur_opp, a.path, a.path_stride = f(), f(), f(), f(), 520
        a.done, a.roll, a.leaf_value = f(), f(), f()
        a.q_slots, a.ctl, a.rep_v, a.rep_p, a.totals = f(), f(), f(), f(), f()
        a.wg_own, a.wg_opp = f(), f()
        if whole:
            a.max_turns = 60
            a.game_own, a.game_opp, a.n_turns = f(), f(), f()
        r = self.ro = _lib.RolloutArgs()
        r.n, r.z, r.table = n_games * width, f(), f()
        v = self.value = _lib.ValueSplitArgs()
        v.own, v.opp, v.n = a.wg_own, a.wg_opp, 0            # (n = 0: not launchable)
        q = self.policy = _lib.PolicySplit3Args()
        q.own, q.opp, q.n = a.wg_own, a.wg_opp, 0
        a.value, a.policy, a.rollout = C.addressof(v), C.addressof(q), C.addressof(r)
        self.spare = [f() for _ in range(8)]                  # (pointers for the fields a case fills in)
        self.wv = self.pk = self.ex = self.cap = self.b = None
        if entry == "wave":
            self.wv = _lib.SearchWaveArgs()
            self.wv.width, self.wv.vloss = width, 1.0
        if entry == "park" or park:
            self.pk = _lib.SearchParkArgs()
            self.pk.park_empties, self.pk.parked, self.pk.stones, self.pk.pass_flg = 20, f(), f(), f()
        if entry == "explore":
            self.ex = _lib.SearchExploreArgs()
            self.ex.explore_turns = 8
        if entry == "cap":
            self.cap = _lib.SearchCapArgs()
            self.cap.n_fast, self.cap.full_per_256, self.cap.explore_turns = 4, 64, 8
        if entry == "arena":
            self.b = Call("persistent", n_games=n_games, who=1)

    def __call__(self):
        L = _lib.lib()
        ref = lambda x: None if x is None else C.byref(x)
        if self.entry in ("explore", "cap") and self.pk is not None:
            x = self.ex if self.entry == "explore" else self.cap
            if x is not None:
                x.park = C.addressof(self.pk)
        a = ref(self.a)
        if self.entry == "persistent":
            rc = L.iago_mcts_search_persistent(a, None)
        elif self.entry == "wave":
            rc = L.iago_mcts_search_wave(a, ref(self.wv), None)
        elif self.entry == "split":
            rc = L.iago_mcts_search_split(a, None, None)     # (no streams: creating them needs a device)
        elif self.entry == "park":
            rc = L.iago_mcts_search_park(a, ref(self.pk), None)
        elif self.entry == "explore":
            rc = L.iago_mcts_search_explore(a, ref(self.ex), None)
        elif self.entry == "cap":
            rc = L.iago_mcts_search_cap(a, ref(self.cap), None)
        else:
            rc = L.iago_mcts_search_arena(a, None if self.b is None else ref(self.b.a), None)
        return rc, L.iago_last_error()


def _set(path, value):
    """A fault: c.<path> = value (path: dotted, from the Call)."""
    def fault(c):
        obj, names = c, path.split(".")
        for n in names[:-1]:
            obj = getattr(obj, n)
        setattr(obj, names[-1], value(c) if callable(value) else value)
    return fault


def _both(*faults):
    def fault(c):
        for f in faults:
            f(c)
    return fault


def _index(path, i, value):
    def fault(c):
        obj = c
        for n in path.split("."):
            obj = getattr(obj, n)
        obj[i] = value
    return fault


P = b"iago_mcts_search_persistent: "
M_NULL = P + b"null args"
M_TREE = P + b"bad tree (the value cache `v` is required)"
M_MANY = P + b"too many games"
M_STATE = P + b"null or misaligned state array"
M_NUM = P + b"n_thr >= 1, n_sims >= 0, 0 <= lmbda <= 1, net_workgroups >= 1 expected"
M_WHOLE = (P + b"whole games (max_turns > 0) need game_own, game_opp, n_turns, and all of rec_own / rec_opp / rec_valid / "
           b"rec_move / rec_pi or none")
M_STREAM = (P + b"games_total >= 0; a stream (games_total > 0) plays whole games (max_turns > 0, n_sims >= 1), without "
            b"z_log or trace")
M_ROOT = P + b"root_own / root_opp expected"
M_ZLOG = P + b"z_log needs z_log_n"
M_RING = b"iago_mcts_search_wave: more slots (n_games x width) than a request ring holds"
M_ROLL = P + b"product-form rollout of the n games without trace / uniforms expected"
M_GPW = P + b"games_per_workgroup is 0 (= 32), 8, 16 or 32"
M_CUS = P + b"max_cus < 0"
M_VT = P + b"vtable must be 32-byte aligned, vtable_slots a power of two"
M_ROWS = (P + b"the nets read their rows from wg_own / wg_opp (four rows per workgroup of the grid: n >= 4 x (game + net "
          b"workgroups)), no gather list, no device count")
M_ARENA_ROWS = (b"iago_mcts_search_arena: each agent's nets read their rows from its wg_own / wg_opp (four rows per "
                b"workgroup of the WHOLE grid: n >= 4 x (both agents' game workgroups + net workgroups)), no gather list, "
                b"no device count")
M_NO_DEVICE = b"iago_mcts_search_capacity: cannot reserve the nets' LDS image"
M_ARENA_SHARED = (b"iago_mcts_search_arena: the two argument sets share a tree, ctl, q_slots, reply or state arrays, or a "
                  b"position table (each agent needs its own)")
M_ARENA_ONE = (b"iago_mcts_search_arena: one search per agent and launch (max_turns 0, games_total 0): a game's two trees "
               b"live in different workgroups")
WHY = {"park": b"a match's policy side needs the net workgroups to its last move",
       "explore": b"a match's moves are not drawn from the visit counts",
       "cap": b"a match's searches are not capped"}

ONE, WHOLE = dict(), dict(whole=True)
spare = lambda i: (lambda c: c.spare[i])

# (id, entry, base, fault, return code, message)
CASES = [
    # ---- check_args, through iago_mcts_search_persistent
    ("null-a", "persistent", ONE, _set("a", None), INVALID, M_NULL),
    ("null-tree", "persistent", ONE, _set("a.tree", None), INVALID, M_NULL),
    ("null-value", "persistent", ONE, _set("a.value", None), INVALID, M_NULL),
    ("null-policy", "persistent", ONE, _set("a.policy", None), INVALID, M_NULL),
    ("null-rollout", "persistent", ONE, _set("a.rollout", None), INVALID, M_NULL),
    ("tree-n_games-0", "persistent", ONE, _set("tree.n_games", 0), INVALID, M_TREE),
    ("tree-capacity-0", "persistent", ONE, _set("tree.capacity", 0), INVALID, M_TREE),
    ("tree-nodes-null", "persistent", ONE, _set("tree.nodes", None), INVALID, M_TREE),
    ("tree-nodes-align-32", "persistent", ONE, _set("tree.nodes", lambda c: c.tree.nodes + 16), INVALID, M_TREE),
    ("tree-n_nodes-null", "persistent", ONE, _set("tree.n_nodes", None), INVALID, M_TREE),
    ("tree-root-null", "persistent", ONE, _set("tree.root", None), INVALID, M_TREE),
    ("tree-overflow-null", "persistent", ONE, _set("tree.overflow", None), INVALID, M_TREE),
    ("tree-no-value-cache", "persistent", ONE, _set("tree.has_v", 0), INVALID, M_TREE),
    ("too-many-games", "persistent", ONE, _set("tree.n_games", 0x7FFFFFF1), INVALID, M_MANY),
] + [
    ("state-%s-null" % k, "persistent", ONE, _set("a." + k, None), INVALID, M_STATE)
    for k in ("active", "cur_node", "cur_own", "cur_opp", "path", "done", "roll", "leaf_value", "q_slots", "ctl", "rep_v",
              "rep_p", "totals", "wg_own", "wg_opp")
] + [
    ("state-path_stride-7", "persistent", ONE, _set("a.path_stride", 7), INVALID, M_STATE),
    ("state-q_slots-align-64", "persistent", ONE, _set("a.q_slots", lambda c: c.a.q_slots + 32), INVALID, M_STATE),
    ("state-rep_p-align-8", "persistent", ONE, _set("a.rep_p", lambda c: c.a.rep_p + 4), INVALID, M_STATE),
    ("state-rep_v-align-8", "persistent", ONE, _set("a.rep_v", lambda c: c.a.rep_v + 4), INVALID, M_STATE),
    ("state-ctl-align-16", "persistent", ONE, _set("a.ctl", lambda c: c.a.ctl + 8), INVALID, M_STATE),
    ("n_thr-0", "persistent", ONE, _set("a.n_thr", 0), INVALID, M_NUM),
    ("n_sims-negative", "persistent", ONE, _set("a.n_sims", -1), INVALID, M_NUM),
    ("lmbda-above-1", "persistent", ONE, _set("a.lmbda", 1.5), INVALID, M_NUM),
    ("lmbda-negative", "persistent", ONE, _set("a.lmbda", -0.25), INVALID, M_NUM),
    ("lmbda-nan", "persistent", ONE, _set("a.lmbda", float("nan")), INVALID, M_NUM),
    ("net_workgroups-0", "persistent", ONE, _set("a.net_workgroups", 0), INVALID, M_NUM),
    ("max_turns-negative", "persistent", ONE, _set("a.max_turns", -1), INVALID, M_WHOLE),
    ("whole-game_own-null", "persistent", WHOLE, _set("a.game_own", None), INVALID, M_WHOLE),
    ("whole-game_opp-null", "persistent", WHOLE, _set("a.game_opp", None), INVALID, M_WHOLE),
    ("whole-n_turns-null", "persistent", WHOLE, _set("a.n_turns", None), INVALID, M_WHOLE),
    ("whole-rec_move-alone", "persistent", WHOLE, _set("a.rec_move", spare(0)), INVALID, M_WHOLE),
    ("whole-rec_pi-missing", "persistent", WHOLE,
     _both(_set("a.rec_move", spare(0)), _set("a.rec_own", spare(1)), _set("a.rec_opp", spare(2)),
           _set("a.rec_valid", spare(3))), INVALID, M_WHOLE),
    ("games_total-negative", "persistent", WHOLE, _set("a.games_total", -1), INVALID, M_STREAM),
    ("stream-of-one-search", "persistent", ONE, _set("a.games_total", 8), INVALID, M_STREAM),
    ("stream-n_sims-0", "persistent", WHOLE, _both(_set("a.games_total", 8), _set("a.n_sims", 0)), INVALID, M_STREAM),
    ("stream-z_log", "persistent", WHOLE, _both(_set("a.games_total", 8), _set("a.z_log", spare(0))), INVALID, M_STREAM),
    ("stream-z_log_rows", "persistent", WHOLE, _both(_set("a.games_total", 8), _set("a.z_log_rows", 4)), INVALID, M_STREAM),
    ("stream-trace", "persistent", WHOLE, _both(_set("a.games_total", 8), _set("a.trace", spare(0))), INVALID, M_STREAM),
    ("stream-trace_rows", "persistent", WHOLE, _both(_set("a.games_total", 8), _set("a.trace_rows", 4)), INVALID, M_STREAM),
    ("root_own-null", "persistent", ONE, _set("a.root_own", None), INVALID, M_ROOT),
    ("root_opp-null", "persistent", ONE, _set("a.root_opp", None), INVALID, M_ROOT),
    ("z_log-null", "persistent", ONE, _set("a.z_log_rows", 4), INVALID, M_ZLOG),
    ("z_log_n-null", "persistent", ONE, _both(_set("a.z_log_rows", 4), _set("a.z_log", spare(0))), INVALID, M_ZLOG),
    ("wave-ring-129x32", "wave", dict(n_games=129, width=32), lambda c: None, CAPACITY, M_RING),
    ("rollout-n", "persistent", ONE, _set("ro.n", 5), INVALID, M_ROLL),
    ("rollout-n-of-a-wave", "wave", dict(n_games=8, width=8), _set("ro.n", 8), INVALID, M_ROLL),
    ("rollout-z-null", "persistent", ONE, _set("ro.z", None), INVALID, M_ROLL),
    ("rollout-table-null", "persistent", ONE, _set("ro.table", None), INVALID, M_ROLL),
    ("rollout-table-align-16", "persistent", ONE, _set("ro.table", lambda c: c.ro.table + 8), INVALID, M_ROLL),
    ("rollout-log_form", "persistent", ONE, _set("ro.log_form", 1), INVALID, M_ROLL),
    ("rollout-trace", "persistent", ONE, _set("ro.trace", spare(0)), INVALID, M_ROLL),
    ("rollout-uniforms", "persistent", ONE, _set("ro.uniforms", spare(0)), INVALID, M_ROLL),
    ("rollout-throughput_hint", "persistent", ONE, _set("ro.throughput_hint", 1), INVALID, M_ROLL),
    ("games_per_workgroup-7", "persistent", ONE, _set("a.games_per_workgroup", 7), INVALID, M_GPW),
    ("games_per_workgroup-7-chain-skip", "persistent", ONE, _set("a.games_per_workgroup", 7 | _lib.SEARCH_CHAIN_SKIP),
     INVALID, M_GPW),
    ("games_per_workgroup-40", "persistent", ONE, _set("a.games_per_workgroup", 40), INVALID, M_GPW),
    ("max_cus-negative", "persistent", ONE, _set("a.max_cus", -1), INVALID, M_CUS),
    ("vtable-null", "persistent", ONE, _set("a.vtable_slots", 1024), INVALID, M_VT),
    ("vtable-align-32", "persistent", ONE,
     _both(_set("a.vtable_slots", 1024), _set("a.vtable", lambda c: c.spare[0] + 16)), INVALID, M_VT),
    ("vtable_slots-not-a-power-of-two", "persistent", ONE,
     _both(_set("a.vtable_slots", 1000), _set("a.vtable", spare(0))), INVALID, M_VT),
    # ---- the entry points' own checks
    ("wave-null-a", "wave", ONE, _set("a", None), INVALID, b"iago_mcts_search_wave: null args"),
    ("wave-null-w", "wave", ONE, _set("wv", None), INVALID, b"iago_mcts_search_wave: null args"),
    ("wave-width-4", "wave", ONE, _set("wv.width", 4), INVALID, b"iago_mcts_search_wave: width is 1, 8, 16 or 32"),
    ("wave-vloss-negative", "wave", ONE, _set("wv.vloss", -1.0), INVALID,
     b"iago_mcts_search_wave: vloss >= 0 (finite) expected"),
    ("wave-vloss-nan", "wave", ONE, _set("wv.vloss", float("nan")), INVALID,
     b"iago_mcts_search_wave: vloss >= 0 (finite) expected"),
    ("wave-vloss-inf", "wave", ONE, _set("wv.vloss", float("inf")), INVALID,
     b"iago_mcts_search_wave: vloss >= 0 (finite) expected"),
    ("wave-whole-games", "wave", WHOLE, lambda c: None, INVALID,
     b"iago_mcts_search_wave: one search per launch (max_turns 0, games_total 0): whole games take "
     b"iago_mcts_search_persistent"),
    ("wave-games_total", "wave", ONE, _set("a.games_total", 8), INVALID,
     b"iago_mcts_search_wave: one search per launch (max_turns 0, games_total 0): whole games take "
     b"iago_mcts_search_persistent"),
    ("wave-check_args", "wave", ONE, _set("a.n_thr", 0), INVALID, M_NUM),
    ("split-null-streams", "split", ONE, lambda c: None, INVALID, b"iago_mcts_search_split: null streams"),
    ("park-null-a", "park", WHOLE, _set("a", None), INVALID, b"iago_mcts_search_park: null args"),
    ("park-null-pk", "park", WHOLE, _set("pk", None), INVALID, b"iago_mcts_search_park: null args"),
    ("explore-null-a", "explore", WHOLE, _set("a", None), INVALID, b"iago_mcts_search_explore: null args"),
    ("explore-null-ex", "explore", WHOLE, _set("ex", None), INVALID, b"iago_mcts_search_explore: null args"),
    ("cap-null-a", "cap", WHOLE, _set("a", None), INVALID, b"iago_mcts_search_cap: null args"),
    ("cap-null-cap", "cap", WHOLE, _set("cap", None), INVALID, b"iago_mcts_search_cap: null args"),
    ("cap-n_fast-0", "cap", WHOLE, _set("cap.n_fast", 0), INVALID, b"iago_mcts_search_cap: n_fast must be in [1, n_sims]"),
    ("cap-n_fast-above-n_sims", "cap", WHOLE, _set("cap.n_fast", 17), INVALID,
     b"iago_mcts_search_cap: n_fast must be in [1, n_sims]"),
    ("cap-full_per_256-0", "cap", WHOLE, _set("cap.full_per_256", 0), INVALID,
     b"iago_mcts_search_cap: full_per_256 must be in [1, 256]"),
    ("cap-full_per_256-257", "cap", WHOLE, _set("cap.full_per_256", 257), INVALID,
     b"iago_mcts_search_cap: full_per_256 must be in [1, 256]"),
]

# ---- what park, explore and cap share: the hand-over's arguments (check_park), the options, self-play only
for who, x in (("park", "pk"), ("explore", "ex"), ("cap", "cap")):
    W = b"iago_mcts_search_" + who.encode()
    CASES += [
        (who + "-reserved", who, WHOLE, _index(x + ".reserved", 2, 1), INVALID, W + b": reserved fields must be 0"),
        (who + "-reserved0", who, WHOLE, _set(x + ".reserved0", 1), INVALID, W + b": reserved fields must be 0"),
        (who + "-one-search", who, ONE, lambda c: None, INVALID, W + b": whole games only (max_turns > 0)"),
        (who + "-match-codes", who, WHOLE, _index("active", 3, _lib.MATCH_MCTS_COLOUR_1), INVALID,
         W + b": match codes in `active` (self-play games only: " + WHY[who] + b")"),
        (who + "-check_args", who, WHOLE, _set("a.n_thr", 0), INVALID, M_NUM),
    ]
    if who != "park":
        CASES += [
            (who + "-explore_turns-negative", who, WHOLE, _set(x + ".explore_turns", -1), INVALID,
             W + b": explore_turns must be in [0, 128]"),
            (who + "-explore_turns-129", who, WHOLE, _set(x + ".explore_turns", 129), INVALID,
             W + b": explore_turns must be in [0, 128]"),
            (who + "-park-streams", who, dict(whole=True, park=True), _set("pk.streams", spare(0)), INVALID,
             W + b" (park): park->streams must be NULL or `streams`"),
        ]
    base = WHOLE if who == "park" else dict(whole=True, park=True)
    W2 = W if who == "park" else W + b" (park)"
    tag = who if who == "park" else who + "-park"
    CASES += [
        (tag + "-%s-null" % k, who, base, _set("pk." + k, None), INVALID, W2 + b": parked, stones and pass_flg expected")
        for k in ("parked", "stones", "pass_flg")
    ] + [
        (tag + "-park_empties-negative", who, base, _set("pk.park_empties", -1), INVALID,
         W2 + b": park_empties must be in [0, 20]"),
        (tag + "-park_empties-21", who, base, _set("pk.park_empties", 21), INVALID, W2 + b": park_empties must be in [0, 20]"),
    ]
    if who != "park":
        CASES += [
            (tag + "-reserved", who, base, _index("pk.reserved", 0, 1), INVALID, W2 + b": reserved fields must be 0"),
            (tag + "-reserved0", who, base, _set("pk.reserved0", 1), INVALID, W2 + b": reserved fields must be 0"),
        ]

# ---- the arena's own rules
CASES += [
    ("arena-null-a", "arena", ONE, _set("a", None), INVALID, b"iago_mcts_search_arena: null args"),
    ("arena-null-b", "arena", ONE, _set("b", None), INVALID, b"iago_mcts_search_arena: null args"),
    ("arena-a-max_turns", "arena", ONE, _set("a.max_turns", 60), INVALID, M_ARENA_ONE),
    ("arena-b-games_total", "arena", ONE, _set("b.a.games_total", 8), INVALID, M_ARENA_ONE),
    ("arena-a-check_args", "arena", ONE, _set("a.n_thr", 0), INVALID, M_NUM),
    ("arena-b-check_args", "arena", ONE, _set("b.tree.has_v", 0), INVALID, M_TREE),
    ("arena-a-match-codes", "arena", ONE, _index("active", 0, _lib.MATCH_MCTS_COLOUR_2), INVALID,
     b"iago_mcts_search_arena: match codes in `active` (0 / 1 expected)"),
    ("arena-b-match-codes", "arena", ONE, _index("b.active", 1, _lib.MATCH_MCTS_COLOUR_1), INVALID,
     b"iago_mcts_search_arena: match codes in `active` (0 / 1 expected)"),
    ("arena-shared-ctl", "arena", ONE, _set("b.a.ctl", lambda c: c.a.ctl), INVALID, M_ARENA_SHARED),
    ("arena-shared-tree", "arena", ONE, _set("b.a.tree", lambda c: c.a.tree), INVALID, M_ARENA_SHARED),
    ("arena-shared-nodes", "arena", ONE, _set("b.tree.nodes", lambda c: c.tree.nodes), INVALID, M_ARENA_SHARED),
    ("arena-shared-z", "arena", ONE, _set("b.ro.z", lambda c: c.ro.z), INVALID, M_ARENA_SHARED),
    ("arena-shared-wg_own", "arena", ONE,
     _both(_set("b.a.wg_own", lambda c: c.a.wg_own), _set("b.value.own", lambda c: c.a.wg_own),
           _set("b.policy.own", lambda c: c.a.wg_own)), INVALID, M_ARENA_SHARED),
    ("arena-shared-vtable", "arena", ONE,
     _both(_set("a.vtable", spare(0)), _set("a.vtable_slots", 1024), _set("b.a.vtable", spare(0)),
           _set("b.a.vtable_slots", 1024)), INVALID, M_ARENA_SHARED),
    ("arena-net_workgroups-1", "arena", ONE, _both(_set("a.net_workgroups", 1), _set("b.a.net_workgroups", 1)), INVALID,
     b"iago_mcts_search_arena: net_workgroups >= 2 expected (a server per agent)"),
]


def test_case_ids_are_unique():
    ids = [c[0] for c in CASES]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("entry,base,fault,rc,msg", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_refusal(entry, base, fault, rc, msg):
    call = Call(entry, **base)
    fault(call)
    assert call() == (rc, msg)


def _unbroken(entry, base):
    """What an unbroken base set answers: never IAGO_OK -- without a device the first device query refuses it, with one
    the nets'-rows check does (value->n = policy->n = 0), after the queries and before anything is zeroed or launched."""
    rc, msg = Call(entry, **base)()
    assert rc != OK
    if _lib.device_count() == 0:
        assert (rc, msg) == (HIP, M_NO_DEVICE)
    else:
        assert (rc, msg) == (INVALID, M_ARENA_ROWS if entry == "arena" else M_ROWS)
    return rc, msg


@pytest.mark.parametrize("entry,base", [("persistent", ONE), ("persistent", WHOLE), ("wave", dict(n_games=8, width=8)),
                                        ("park", WHOLE), ("explore", WHOLE), ("explore", dict(whole=True, park=True)),
                                        ("cap", WHOLE), ("cap", dict(whole=True, park=True)), ("arena", ONE)],
                         ids=["persistent", "whole-games", "wave", "park", "explore", "explore-park", "cap", "cap-park",
                              "arena"])
def test_no_base_set_can_be_launched(entry, base):
    _unbroken(entry, base)


def test_the_wave_takes_any_games_per_workgroup():
    """games_per_workgroup is the single search's: the wave search (32 slots per workgroup) does not look at it."""
    base = dict(n_games=8, width=8)
    call = Call("wave", **base)
    call.a.games_per_workgroup = 7
    assert call() == _unbroken("wave", base)


def test_the_same_streams_in_both_places_pass_the_option_checks():
    """park->streams == streams is allowed: with both NULL the call goes on to the device queries like the base set."""
    for entry in ("explore", "cap"):
        base = dict(whole=True, park=True)
        call = Call(entry, **base)
        call.pk.streams = None
        assert call() == _unbroken(entry, base)
