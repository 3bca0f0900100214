"""The refusals of the lane searches' host layer (csrc/endgame_kernel.hip, csrc/alphabeta_kernel.hip), without a GPU:
every case starts from a valid argument set for one of the seven entry points, breaks ONE thing (a few: two, to anchor
the order of the checks), calls the entry point and pins the exact return code and the exact iago_last_error() text --
so that whoever restates that layer sees which check was lost or moved.  One case per refusal that is reached before
the first device call, and for the null-pointer conditions one case per pointer.

Nothing here can be launched, on any machine: every device pointer is a made-up constant that is never dereferenced,
no case calls an entry point with an unbroken argument set or with n == 0 (those go on to the device), and
test_every_case_breaks_its_base_set holds the table to that."""
import ctypes as C

import pytest

from iago_amd import _lib

INVALID = _lib.IAGO_ERR_INVALID

FAKE = 0x7E0000000000   # never dereferenced: the refusals under test come before any use of it
N = 4

JOB_ARRAYS = ("job_own", "job_opp", "job_root", "job_path", "job_score", "job_move", "job_nodes", "job_done")
SOLVE_PTRS = ("own", "opp", "score", "move", "nodes", "solved", "ctl")
SEARCH_PTRS = ("own", "opp", "score", "move", "nodes", "done", "ctl")
SPLIT_PTRS = ("own", "opp", "job_count", "job_first", "ctl")
PLAY_PTRS = ("own", "opp", "turn", "stones", "pass_flg", "parked", "rec_own", "rec_opp", "rec_valid", "rec_move",
             "rec_score", "finished", "ctl")

# entry -> (symbol, argument struct, its pointers, its other fields)
ENTRIES = {
    "solve": ("iago_solve_endgame", _lib.EndgameArgs, SOLVE_PTRS,
              dict(n=N, mode=_lib.ENDGAME_EXACT, max_empties=20, time_limit_ms=1000)),
    "moves": ("iago_solve_endgame_moves", _lib.EndgameMovesArgs, SOLVE_PTRS + ("best",),
              dict(n=N, mode=_lib.ENDGAME_WLD, moves=_lib.ENDGAME_MOVES_BEST, max_empties=20, time_limit_ms=1000)),
    "moves-all": ("iago_solve_endgame_moves", _lib.EndgameMovesArgs, SOLVE_PTRS + ("best", "move_score"),
                  dict(n=N, mode=_lib.ENDGAME_EXACT, moves=_lib.ENDGAME_MOVES_ALL, max_empties=20, time_limit_ms=1000)),
    "solve-split": ("iago_solve_endgame_split", _lib.EndgameSplitArgs,
                    SOLVE_PTRS + ("best", "move_score", "job_count", "job_first") + JOB_ARRAYS,
                    dict(n=N, mode=_lib.ENDGAME_EXACT, split=2, max_empties=20, time_limit_ms=1000, job_capacity=64)),
    "play": ("iago_play_endgame", _lib.PlayEndgameArgs, PLAY_PTRS,
             dict(n=N, stride=N, max_turns=60, max_empties=20, time_limit_ms=1000)),
    "play-moves": ("iago_play_endgame_moves", _lib.PlayEndgameMovesArgs, None, None),
    "search": ("iago_alphabeta_moves", _lib.AlphaBetaArgs, SEARCH_PTRS, dict(n=N, depth=4, time_limit_ms=1000)),
    "search-split": ("iago_alphabeta_moves_split", _lib.AlphaBetaSplitArgs,
                     SEARCH_PTRS + ("job_count", "job_first") + JOB_ARRAYS,
                     dict(n=N, depth=4, split=2, time_limit_ms=1000, job_capacity=64)),
}
WHO = {k: v[0].encode() for k, v in ENTRIES.items()}


def _fill(a, pointers, fields, first=1):
    for i, k in enumerate(pointers):
        setattr(a, k, FAKE + (first + i) * 0x1000)
    for k, v in fields.items():
        setattr(a, k, v)


class Call(object):
    """A valid call of one entry point; `a` is the argument struct (None: a null one)."""

    def __init__(self, entry):
        self.symbol, struct, pointers, fields = ENTRIES[entry]
        self.a = struct()
        if entry == "play-moves":
            _fill(self.a.play, PLAY_PTRS, ENTRIES["play"][3])
            self.a.rec_best = FAKE + 0x100000
        else:
            _fill(self.a, pointers, fields)

    def image(self):
        return None if self.a is None else bytes(self.a)

    def __call__(self):
        L = _lib.lib()
        rc = getattr(L, self.symbol)(None if self.a is None else C.byref(self.a), None)
        return rc, L.iago_last_error()


def _set(path, value):
    """A fault: c.<path> = value (path: dotted, from the Call)."""
    def fault(c):
        obj, names = c, path.split(".")
        for n in names[:-1]:
            obj = getattr(obj, n)
        setattr(obj, names[-1], value)
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


NO_JOB_ARRAYS = _both(*[_set("a." + k, None) for k in JOB_ARRAYS])

T_NULL = b": null pointer or negative n"
T_NULL_SPLIT = b": null pointer, negative n or n above 2^31 - 1"
T_MODE = b": mode must be IAGO_ENDGAME_EXACT or IAGO_ENDGAME_WLD"
T_MOVES = b": moves must be IAGO_ENDGAME_MOVES_BEST or IAGO_ENDGAME_MOVES_ALL"
T_EMPTIES = b": max_empties must be in [0, 20]"
T_TIME = b": time_limit_ms must be in [1, 600000]"
T_CAPACITY = b": job_capacity must be in [0, 2^31 - 1]"
T_ARRAYS = b": the job arrays are all given, or all null with job_capacity 0 (the count-only form)"
T_RESERVED = b": reserved fields must be 0"
T_SOLVE_SPLIT = b": split must be 1 or 2"
T_SEARCH_SPLIT = b": split must be 1 or 2 and below depth"
T_STRIDE = b": stride >= n expected"
T_TURNS = b": max_turns must be in [1, IAGO_MAX_TURNS]"

# (id, entry, fault, text after the entry point's name)
CASES = []


def case(tag, entry, fault, text):
    CASES.append((entry + "-" + tag, entry, fault, WHO[entry] + text))


for e in ENTRIES:
    case("null-args", e, _set("a", None), b": null args")

# ---- the null-pointer conditions, one case per pointer, and n
for e, pointers, text in (("solve", SOLVE_PTRS, T_NULL), ("moves", SOLVE_PTRS + ("best",), T_NULL),
                          ("solve-split", SPLIT_PTRS, T_NULL_SPLIT), ("play", PLAY_PTRS, T_NULL),
                          ("search", SEARCH_PTRS, T_NULL), ("search-split", SPLIT_PTRS, T_NULL_SPLIT)):
    for k in pointers:
        case("null-" + k, e, _set("a." + k, None), text)
    case("n-negative", e, _set("a.n", -1), text)
for k in PLAY_PTRS:
    case("null-" + k, "play-moves", _set("a.play." + k, None), T_NULL)
case("null-rec_best", "play-moves", _set("a.rec_best", None), T_NULL)
case("n-negative", "play-moves", _set("a.play.n", -1), T_NULL)
for e in ("solve-split", "search-split"):
    case("n-2^31", e, _set("a.n", 2 ** 31), T_NULL_SPLIT)

# ---- the entries' own fields
for e in ("solve", "moves", "solve-split"):
    case("mode-negative", e, _set("a.mode", -1), T_MODE)
    case("mode-2", e, _set("a.mode", 2), T_MODE)
case("moves-negative", "moves", _set("a.moves", -1), T_MOVES)
case("moves-2", "moves", _set("a.moves", 2), T_MOVES)
case("move_score-under-best", "moves", _set("a.move_score", FAKE), b": move_score must be NULL under IAGO_ENDGAME_MOVES_BEST")
case("move_score-missing", "moves-all", _set("a.move_score", None),
     b": move_score is required under IAGO_ENDGAME_MOVES_ALL")
case("depth-0", "search", _set("a.depth", 0), b": depth must be in [1, 10]")
case("depth-11", "search", _set("a.depth", 11), b": depth must be in [1, 10]")
case("depth-1", "search-split", _set("a.depth", 1), b": depth must be in [2, 10]")
case("depth-11", "search-split", _set("a.depth", 11), b": depth must be in [2, 10]")
for e, text in (("solve-split", T_SOLVE_SPLIT), ("search-split", T_SEARCH_SPLIT)):
    case("split-0", e, _set("a.split", 0), text)
    case("split-negative", e, _set("a.split", -1), text)
    case("split-3", e, _set("a.split", 3), text)
case("split-at-depth", "search-split", _both(_set("a.depth", 2), _set("a.split", 2)), T_SEARCH_SPLIT)
for e, at in (("play", "a."), ("play-moves", "a.play.")):
    case("stride-below-n", e, _set(at + "stride", N - 1), T_STRIDE)
    case("max_turns-0", e, _set(at + "max_turns", 0), T_TURNS)
    case("max_turns-129", e, _set(at + "max_turns", 129), T_TURNS)

# ---- what they share: max_empties, time_limit_ms, reserved
AT = {e: "a.play." if e == "play-moves" else "a." for e in ENTRIES}
for e in ("solve", "moves", "solve-split", "play", "play-moves"):
    case("max_empties-negative", e, _set(AT[e] + "max_empties", -1), T_EMPTIES)
    case("max_empties-21", e, _set(AT[e] + "max_empties", 21), T_EMPTIES)
for e in ENTRIES:
    case("time_limit_ms-0", e, _set(AT[e] + "time_limit_ms", 0), T_TIME)
    case("time_limit_ms-600001", e, _set(AT[e] + "time_limit_ms", 600001), T_TIME)
    for i in range(4):
        case("reserved-%d" % i, e, _index(AT[e] + "reserved", i, 1), T_RESERVED)
for e in ("solve", "play", "play-moves", "search-split"):
    case("reserved0", e, _set(AT[e] + "reserved0", 1), T_RESERVED)
for i in range(4):
    case("own-reserved-%d" % i, "play-moves", _index("a.reserved", i, 1), T_RESERVED)

# ---- the split entries: the job arrays and the outputs of the full form
for e, done in (("solve-split", "solved"), ("search-split", "done")):
    case("job_capacity-negative", e, _set("a.job_capacity", -1), T_CAPACITY)
    case("job_capacity-2^31", e, _set("a.job_capacity", 2 ** 31), T_CAPACITY)
    for k in JOB_ARRAYS:
        case("seven-arrays-no-" + k, e, _set("a." + k, None), T_ARRAYS)
    case("one-array", e, _both(NO_JOB_ARRAYS, _set("a.job_done", FAKE), _set("a.job_capacity", 0)), T_ARRAYS)
    case("no-arrays-job_capacity-1", e, _both(NO_JOB_ARRAYS, _set("a.job_capacity", 1)), T_ARRAYS)
    for k in ("score", "move", "nodes", done):
        case("full-form-null-" + k, e, _set("a." + k, None), b": null score, move, nodes or " + done.encode())

# ---- two faults at once: the earlier check wins
case("null-own+mode", "solve", _both(_set("a.own", None), _set("a.mode", 2)), T_NULL)
case("mode+max_empties", "solve", _both(_set("a.mode", 2), _set("a.max_empties", 21)), T_MODE)
case("max_empties+time_limit_ms", "solve", _both(_set("a.max_empties", 21), _set("a.time_limit_ms", 0)), T_EMPTIES)
case("time_limit_ms+reserved", "solve", _both(_set("a.time_limit_ms", 0), _index("a.reserved", 0, 1)), T_TIME)
case("null-best+mode", "moves", _both(_set("a.best", None), _set("a.mode", 2)), T_NULL)
case("mode+moves", "moves", _both(_set("a.mode", 2), _set("a.moves", 2)), T_MODE)
case("moves+move_score", "moves", _both(_set("a.moves", 2), _set("a.move_score", FAKE)), T_MOVES)
case("move_score+max_empties", "moves", _both(_set("a.move_score", FAKE), _set("a.max_empties", 21)),
     b": move_score must be NULL under IAGO_ENDGAME_MOVES_BEST")
case("null-ctl+mode", "solve-split", _both(_set("a.ctl", None), _set("a.mode", 2)), T_NULL_SPLIT)
case("mode+split", "solve-split", _both(_set("a.mode", 2), _set("a.split", 3)), T_MODE)
case("split+time_limit_ms", "solve-split", _both(_set("a.split", 3), _set("a.time_limit_ms", 0)), T_SOLVE_SPLIT)
case("split+max_empties", "solve-split", _both(_set("a.split", 0), _set("a.max_empties", 21)), T_SOLVE_SPLIT)
case("max_empties+time_limit_ms", "solve-split", _both(_set("a.max_empties", -1), _set("a.time_limit_ms", 0)), T_EMPTIES)
case("null-job_count+depth", "search-split", _both(_set("a.job_count", None), _set("a.depth", 1)), T_NULL_SPLIT)
case("depth+split", "search-split", _both(_set("a.depth", 11), _set("a.split", 3)), b": depth must be in [2, 10]")
case("split+time_limit_ms", "search-split", _both(_set("a.split", 3), _set("a.time_limit_ms", 0)), T_SEARCH_SPLIT)
for e, done in (("solve-split", "solved"), ("search-split", "done")):
    case("time_limit_ms+job_capacity", e, _both(_set("a.time_limit_ms", 600001), _set("a.job_capacity", -1)), T_TIME)
    case("job_capacity+seven-arrays", e, _both(_set("a.job_capacity", 2 ** 31), _set("a.job_path", None)), T_CAPACITY)
    case("seven-arrays+null-score", e, _both(_set("a.job_own", None), _set("a.score", None)), T_ARRAYS)
    case("null-" + done + "+reserved", e, _both(_set("a." + done, None), _index("a.reserved", 3, 1)),
         b": null score, move, nodes or " + done.encode())
case("null-done+reserved0", "search-split", _both(_set("a.done", None), _set("a.reserved0", 1)),
     b": null score, move, nodes or done")
for e in ("play", "play-moves"):
    case("null-parked+stride", e, _both(_set(AT[e] + "parked", None), _set(AT[e] + "stride", 0)), T_NULL)
    case("stride+max_turns", e, _both(_set(AT[e] + "stride", 0), _set(AT[e] + "max_turns", 0)), T_STRIDE)
    case("max_turns+max_empties", e, _both(_set(AT[e] + "max_turns", 129), _set(AT[e] + "max_empties", 21)), T_TURNS)
    case("max_empties+time_limit_ms", e, _both(_set(AT[e] + "max_empties", 21), _set(AT[e] + "time_limit_ms", 0)),
         T_EMPTIES)
    case("time_limit_ms+reserved0", e, _both(_set(AT[e] + "time_limit_ms", 0), _set(AT[e] + "reserved0", 1)), T_TIME)
case("null-rec_best+stride", "play-moves", _both(_set("a.rec_best", None), _set("a.play.stride", 0)), T_NULL)
case("time_limit_ms+own-reserved", "play-moves", _both(_set("a.play.time_limit_ms", 0), _index("a.reserved", 1, 1)),
     T_TIME)
case("null-done+depth", "search", _both(_set("a.done", None), _set("a.depth", 0)), T_NULL)
case("depth+time_limit_ms", "search", _both(_set("a.depth", 0), _set("a.time_limit_ms", 0)), b": depth must be in [1, 10]")
case("time_limit_ms+reserved", "search", _both(_set("a.time_limit_ms", 0), _index("a.reserved", 2, 1)), T_TIME)


def test_case_ids_are_unique():
    ids = [c[0] for c in CASES]
    assert len(set(ids)) == len(ids)


def test_every_case_breaks_its_base_set():
    """No case reaches a device call: none calls with its base set as it stands, and none with n == 0."""
    for tag, entry, fault, _ in CASES:
        call = Call(entry)
        base = call.image()
        fault(call)
        assert call.image() != base, tag
        if call.a is not None:
            assert (call.a.play.n if entry == "play-moves" else call.a.n) != 0, tag


@pytest.mark.parametrize("entry,fault,msg", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_refusal(entry, fault, msg):
    call = Call(entry)
    fault(call)
    assert call() == (INVALID, msg)
