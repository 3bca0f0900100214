"""The rule of the fixed-depth alpha-beta opponent (tests/alphabeta_ref.py) against itself -- a plain minimax and an
alpha-beta with the root's tie rule -- and against the exact endgame references where the depth reaches the end of the
game; the evaluation's symmetry and bounds; the opening draw; the ABI entries and every refusal that needs no GPU."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from . import alphabeta_ref as ab
from . import endgame_ref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = 0xFFFFFFFFFFFFFFFF


@pytest.fixture(scope="module")
def positions():
    return ab.position_set()


def test_position_set_holds_every_kind(positions):
    own, opp = positions
    assert len(own) == 48
    must_pass, over, inside = ab.kind_counts(own, opp, 3)
    assert must_pass >= 4 and over >= 2 and inside >= 4, (must_pass, over, inside)
    e = [er.empties(a, b) for a, b in zip(own, opp)]
    assert min(e) == 0 and max(e[:24]) >= 48


def test_minimax_equals_alphabeta(positions):
    own, opp = positions
    differ = 0
    for a, b in zip(own, opp):
        got = [ab.alphabeta(a, b, d) for d in (1, 2, 3)]
        assert got == [ab.minimax(a, b, d) for d in (1, 2, 3)], (hex(a), hex(b))
        differ += got[0][1] != got[2][1]
    assert differ >= 8   # depth matters: depth 1 and depth 3 choose different moves


def test_minimax_equals_alphabeta_at_depth_4(positions):
    own, opp = positions
    # 16 of the 48: every third one, so that midgame, late and hand-made boards are among them
    for a, b in list(zip(own, opp))[::3]:
        assert ab.alphabeta(a, b, 4) == ab.minimax(a, b, 4), (hex(a), hex(b))


def _sym(k, x):
    """Board symmetry k (0..7) of the bit mask x: transpose when k & 4, then flip rows when k & 1, columns when k & 2."""
    out = 0
    for a in range(64):
        if (x >> a) & 1:
            r, c = divmod(a, 8)
            if k & 4:
                r, c = c, r
            if k & 1:
                r = 7 - r
            if k & 2:
                c = 7 - c
            out |= 1 << (8 * r + c)
    return out


def test_classes_partition_the_board_and_are_symmetric(positions):
    masks = [m for _, m in ab.CLASSES]
    assert sum(masks) == FULL and all(masks[i] & masks[j] == 0 for i in range(7) for j in range(i))
    assert len({_sym(k, 0x0000000000010203) for k in range(8)}) == 8   # eight different symmetries
    for k in range(8):
        assert [_sym(k, m) for m in masks] == masks
    own, opp = positions
    for a, b in list(zip(own, opp))[:12]:
        for k in range(8):
            assert ab.evaluate(_sym(k, a), _sym(k, b)) == ab.evaluate(a, b)
        assert ab.evaluate(b, a) == -ab.evaluate(a, b)


def test_value_bounds(positions):
    # the table's bound: one side on every square of positive weight, the other on every negative one; mobility 8 * 64
    pos = sum(v * bin(m).count("1") for v, m in ab.CLASSES if v > 0)
    neg = -sum(v * bin(m).count("1") for v, m in ab.CLASSES if v < 0)
    assert (pos, neg) == (520, 408) and pos + neg + 8 * 64 < 10000
    assert ab.terminal(FULL, 0) == 16400 and ab.terminal(0, FULL) == -16400 and ab.terminal(1, 2) == 0
    assert ab.terminal(3, 4) == 10100 and ab.terminal(4, 3) == -10100
    own, opp = positions
    for a, b in zip(own, opp):
        assert abs(ab.evaluate(a, b)) < 10000 and abs(ab.terminal(a, b)) <= 16400
        assert abs(ab.alphabeta(a, b, 2)[0]) <= 16400


def _exact(score):
    return 10000 * ((score > 0) - (score < 0)) + 100 * score


def test_depth_to_the_end_is_the_exact_solver(positions):
    from .conftest import load_json
    rows = [(r["own"], r["opp"]) for r in load_json("endgame_deep.json")["rows"] if r["empties"] <= 7 and r["exact"]]
    assert len(rows) >= 12
    for a, b in rows:
        s, m = er.solve_bits(a, b)
        assert ab.alphabeta(a, b, er.empties(a, b) or 1) == (_exact(s), m), (hex(a), hex(b))
    fixture = {(r["own"], r["opp"]): r["exact"][:2] for r in load_json("endgame_deep.json")["rows"] if r["exact"]}
    for a, b in rows:
        assert list(er.solve_bits(a, b)) == fixture[(a, b)]
    o, p = er.late_positions(24, 4, 0, 8)
    kinds = set()
    for a, b in zip(o, p):
        s, m = er.solve_bits(a, b)
        kinds.add(min(m, 0))
        for extra in (0, 2):   # depth >= empties: more depth changes nothing
            assert ab.alphabeta(a, b, max(er.empties(a, b), 1) + extra) == (_exact(s), m), (hex(int(a)), hex(int(b)))
    assert kinds == {0, -1, -2}


def test_random_move_index_and_pairing():
    rs = np.random.RandomState(1)
    for K in range(1, 34):
        for w in [0, 1, 0xFFFFFFFF, 0x80000000] + [int(x) for x in rs.randint(0, 2 ** 32, 40, dtype=np.int64)]:
            assert 0 <= ab.random_index(w, K) < K
    assert ab.OPENING_KEY == 0x4F50454E == int.from_bytes(b"OPEN", "big")
    from oracle import oracle as orc
    for seed, g, t in ((7, 3, 0), (7, 3, 5), (2 ** 63 + 11, 2 ** 32 - 1, 15)):
        assert ab.word(seed, g, t) == int(orc.philox(seed ^ (0x4F50454E << 32), g, t >> 2, 0, 0)[t & 3])
    # a paired match of B games: g and g + B / 2 draw with the same id, games of one half with different ones
    B = 16
    ids = [ab.opening_id(g, 40, B // 2) for g in range(B)]
    assert ids[:8] == ids[8:] == list(range(40, 48))
    assert [ab.opening_id(g, 40, B) for g in range(B)] == list(range(40, 56))
    own, opp = 0x0000000810000000, 0x0000001008000000
    for t in range(4):
        assert [ab.random_move(own, opp, 9, g, 40, 8, t) for g in range(8)] == \
            [ab.random_move(own, opp, 9, g + 8, 40, 8, t) for g in range(8)]
    assert ab.random_move(1, 4, 9, 0, 0, 1, 0) == -1   # no legal move


def test_random_move_is_uniform():
    own, opp = 0x0000000810000000, 0x0000001008000000   # the start: 4 legal moves
    moves = ab.moves_of(own, opp)
    assert moves == [19, 26, 37, 44]
    n = 4096
    counts = {m: 0 for m in moves}
    for g in range(n):
        counts[ab.random_move(own, opp, 2024, g, 0, n, g % 16)] += 1
    se = (n * 0.25 * 0.75) ** 0.5
    assert all(abs(c - n / 4) <= 5 * se for c in counts.values()), counts


def test_serving_header_lists_the_opponent():
    from iago_amd import _lib
    text = open(os.path.join(ROOT, "include", "iago_hip_serving.h")).read()
    declared = set(re.findall(r"IAGO_API[^;(]*?\b(iago_\w+)\s*\(", text))
    L = _lib.lib()
    for name in ("iago_alphabeta_moves", "iago_random_moves"):
        assert name in declared and name in _lib.SERVING_SYMBOLS and hasattr(L, name), name
    assert C.sizeof(_lib.AlphaBetaArgs) == 8 * 3 + 4 * 2 + 8 * 5 + 8 * 4
    assert re.search(r"#define\s+IAGO_ALPHABETA_MAX_DEPTH\s+10\b", text) and _lib.ALPHABETA_MAX_DEPTH == 10
    assert "#define IAGO_OPENING_KEY 0x4F50454Eu" in text and _lib.OPENING_KEY == ab.OPENING_KEY
    assert _lib.OPENING_SEED_XOR == _lib.OPENING_KEY << 32
    assert _lib.OPENING_KEY not in (_lib.MATCH_KEY, _lib.EXPLORE_KEY, _lib.CAP_KEY, _lib.NOISE_KEY, 0x52504C59)
    assert _lib.REC_OPENING == 5 and _lib.REC_DRAWN == 2
    assert L.iago_abi_version() == 13
    for v, m in ab.CLASSES:   # the header states the rule: every class is in it
        assert "0x%016X" % m in text and re.search(r"%d\s+0x%016X" % (v, m), text), (v, hex(m))


def test_host_side_refusals():
    from iago_amd import _lib
    L = _lib.lib()
    buf = (C.c_uint64 * 8)()
    ctl = (C.c_uint32 * 4)()

    def args(**kw):
        a = _lib.AlphaBetaArgs()
        for f in ("own", "opp", "score", "move", "nodes", "done"):
            setattr(a, f, C.addressof(buf))
        a.ctl = C.addressof(ctl)
        a.n, a.depth, a.time_limit_ms = 1, 4, 1000
        for k, v in kw.items():
            if k == "reserved":
                a.reserved[2] = v
            else:
                setattr(a, k, v)
        return a

    assert L.iago_alphabeta_moves(None, None) == _lib.IAGO_ERR_INVALID
    for kw in (dict(own=None), dict(opp=None), dict(score=None), dict(move=None), dict(nodes=None), dict(done=None),
               dict(ctl=None), dict(n=-1), dict(depth=0), dict(depth=11), dict(depth=-1), dict(time_limit_ms=0),
               dict(time_limit_ms=600001), dict(reserved=7)):
        assert L.iago_alphabeta_moves(C.byref(args(**kw)), None) == _lib.IAGO_ERR_INVALID, kw
        assert b"iago_alphabeta_moves" in L.iago_last_error()
    p = C.addressof(buf)
    for a in ((None, p, 1, 0, 0, 1, 0, p), (p, None, 1, 0, 0, 1, 0, p), (p, p, 1, 0, 0, 1, 0, None), (p, p, -1, 0, 0, 1, 0, p),
              (p, p, 1, 0, 0, 0, 0, p), (p, p, 1, 0, 0, 1, -1, p), (p, p, 1, 0, 0, 1, 128, p)):
        assert L.iago_random_moves(*a, None) == _lib.IAGO_ERR_INVALID, a
        assert b"iago_random_moves" in L.iago_last_error()
    assert L.iago_random_moves(None, None, 0, 0, 0, 1, 0, None, None) == _lib.IAGO_OK   # nothing to do


def test_python_entry_points_refuse_bad_options():
    import torch
    from iago_amd import _lib, engine, ops
    t = torch.zeros(2, dtype=torch.int64)
    for bad in (0, 11, -1, 2.0, True, "4", None):
        with pytest.raises(ValueError, match="depth"):
            ops.alphabeta_moves(t, t, bad)
        with pytest.raises(ValueError, match="depth"):
            engine.AlphaBeta(bad)
    with pytest.raises(ValueError):
        ops.alphabeta_moves(t, t[:1], 2)
    with pytest.raises(_lib.IagoError):
        ops.alphabeta_moves(t, t, 2)                           # CPU tensors: no CPU fallback
    with pytest.raises(_lib.IagoError):
        ops.random_moves(t, t, 1, 0, 2, 0)
    assert engine.AlphaBeta(10).depth == 10 and engine.AlphaBeta(3) == engine.AlphaBeta(3)


class _StubMcts(object):
    """What SelfPlayEngine reads before its first device call; anything else is a failure of the test."""
    n_games = 4

    def __getattr__(self, name):
        raise AssertionError("play_match must check its arguments before the engine is touched (read %r)" % name)


def test_play_match_refusals_before_the_device():
    from iago_amd.engine import AlphaBeta, SelfPlayEngine
    e = SelfPlayEngine(_StubMcts())
    for bad in (1, 3, 18, -2, 2.0, True, "4", None):
        with pytest.raises(ValueError, match="opening_turns"):
            e.play_match(24, opening_turns=bad)
    for bad in (2, "depth 2", types.SimpleNamespace(depth=2), (2,)):
        with pytest.raises(ValueError, match="opponent"):
            e.play_match(24, opponent=bad)
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="paired"):
            e.play_match(24, paired=bad)
    for colour in (1, 2):
        with pytest.raises(ValueError, match="paired"):
            e.play_match(24, mcts_colour=colour, paired=True, opponent=AlphaBeta(2))
    with pytest.raises(ValueError, match="forced_playouts"):
        e.play_match(24, opponent=AlphaBeta(2), forced_playouts=512)
    with pytest.raises(ValueError, match="solve_empties"):
        e.play_match(24, opponent=AlphaBeta(2), solve_empties=21)
    odd = _StubMcts()
    odd.n_games = 5
    with pytest.raises(ValueError, match="even"):
        SelfPlayEngine(odd).play_match(24, paired=True)
