"""The arena without a GPU: the library exports iago_mcts_search_arena and the serving header declares it;
ArenaResult.score() on hand-made tensors; ArenaEngine's default colours and every ValueError of its constructor and of
play's arguments (on stand-ins for the two engines: the checks read attributes only)."""
import os
import re
import subprocess
import types

import pytest
import torch

from iago_amd import _lib, build, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_and_header_declares_the_entry_point():
    out = subprocess.check_output(["nm", "-D", "--defined-only", build.build()]).decode()
    assert re.search(r" T iago_mcts_search_arena$", out, re.M)
    text = open(os.path.join(ROOT, "include", "iago_hip_serving.h")).read()
    assert re.search(r"IAGO_API int iago_mcts_search_arena\(const iago_mcts_search_args \*\w+, "
                     r"const iago_mcts_search_args \*\w+, void \*stream\);", text)
    assert "iago_mcts_search_arena" in _lib.SERVING_SYMBOLS and hasattr(_lib.lib(), "iago_mcts_search_arena")
    assert "iago_mcts_search_arena" not in open(os.path.join(ROOT, "include", "iago_hip.h")).read()
    assert _lib.lib().iago_abi_version() == _lib.ABI_VERSION == 13
    # (host-side refusal, no device needed)
    assert _lib.lib().iago_mcts_search_arena(None, None, None) == _lib.IAGO_ERR_INVALID
    assert b"iago_mcts_search_arena" in _lib.lib().iago_last_error()


def _result(z, a_colour):
    r = engine.ArenaResult()
    r.z = torch.tensor(z, dtype=torch.int8)
    r.a_colour = torch.tensor(a_colour, dtype=torch.int8)
    return r


def test_score_is_from_a_side():
    # z is colour 1's result: A wins where it played the winning colour
    s = _result([1, 1, -1, -1, 0, 0, 1], [1, 2, 1, 2, 1, 2, 1]).score()
    assert s == dict(wins=3, draws=2, losses=2, n=7, win_rate=(3 + 0.5 * 2) / 7)
    assert _result([1, -1, 0], [1, 1, 1]).score() == dict(wins=1, draws=1, losses=1, n=3, win_rate=0.5)
    assert _result([1, -1, 0], [2, 2, 2]).score() == dict(wins=1, draws=1, losses=1, n=3, win_rate=0.5)
    assert _result([1, 1], [2, 2]).score()["win_rate"] == 0.0 and _result([-1, -1], [2, 2]).score()["win_rate"] == 1.0
    empty = _result([], []).score()
    assert empty["n"] == 0 and empty["win_rate"] != empty["win_rate"]


def test_tuples_of_one_agent_on_hand_made_records():
    r = _result([1, -1], [1, 2])
    r.mover = [1, 2]
    r.valid = torch.tensor([[1, 1], [1, 0]], dtype=torch.uint8)
    r.agent = torch.tensor([[0, 1], [1, 0]], dtype=torch.uint8)
    r.own = torch.tensor([[10, 11], [12, 13]])
    r.opp = torch.tensor([[20, 21], [22, 23]])
    r.move = torch.tensor([[3, 4], [5, -1]], dtype=torch.int8)
    r.pi = torch.arange(2 * 2 * 64, dtype=torch.int32).reshape(2, 2, 64)
    assert r.tuples()["own"].tolist() == [10, 11, 12]
    assert r.tuples(agent=0)["own"].tolist() == [10] and r.tuples(agent=1)["own"].tolist() == [11, 12]
    assert r.tuples(agent=1)["z"].tolist() == [-1, -1]          # (from the mover's view)
    assert r.valid.tolist() == [[1, 1], [1, 0]]                 # (left as it was)
    for bad in (2, -1, True, "a"):
        with pytest.raises(ValueError, match="agent"):
            r.tuples(agent=bad)


def _stub(n_games=6, **kw):
    m = types.SimpleNamespace(persistent=True, wave=1, wave_entry=False, n_games=n_games, tree=object(),
                              cur_own=torch.zeros(n_games, dtype=torch.int64))
    m.__dict__.update(kw)
    return m


def test_constructor_refusals_name_the_argument():
    ok = _stub()
    engine.ArenaEngine(ok, _stub())
    cases = [((_stub(persistent=False), _stub()), "mcts_a"), ((ok, _stub(persistent=False)), "mcts_b"),
             ((_stub(wave=8), _stub()), "mcts_a"), ((ok, _stub(wave=8)), "mcts_b"),
             ((ok, _stub(wave_entry=True)), "mcts_b"), ((object(), _stub()), "mcts_a"),
             ((ok, ok), "mcts_b"), ((ok, _stub(tree=ok.tree)), "mcts_b"), ((ok, _stub(n_games=8)), "mcts_b"),
             ((ok, _stub(cur_own=torch.zeros(6, dtype=torch.int64, device="meta"))), "mcts_b")]
    for args, name in cases:
        with pytest.raises(ValueError, match=name):
            engine.ArenaEngine(*args)
    for bad in (0, -1, 129, 2.0, True, None):
        with pytest.raises(ValueError, match="max_turns"):
            engine.ArenaEngine(ok, _stub(), max_turns=bad)
    assert engine.ArenaEngine(ok, _stub(), max_turns=60).max_turns == 60


def test_default_colours_are_halves():
    for B, want in ((6, [1, 1, 1, 2, 2, 2]), (5, [1, 1, 2, 2, 2]), (1, [2])):
        e = engine.ArenaEngine(_stub(B), _stub(B))
        col = e._colours(None)
        assert col.dtype == torch.int8 and col.tolist() == want
    e = engine.ArenaEngine(_stub(4), _stub(4))
    assert e._colours(1).tolist() == [1] * 4 and e._colours(2).tolist() == [2] * 4
    assert e._colours(torch.tensor([2, 1, 1, 2])).tolist() == [2, 1, 1, 2]


def test_play_argument_refusals():
    e = engine.ArenaEngine(_stub(4), _stub(4))
    for bad in (0, 3, True, 1.0, "1", torch.tensor([1, 2, 1]), torch.tensor([1.0, 2.0, 1.0, 2.0]),
                torch.tensor([1, 2, 3, 1]), torch.tensor([[1, 2, 1, 2]]), torch.tensor([0, 1, 2, 1])):
        with pytest.raises(ValueError, match="a_colour"):
            e.play(16, a_colour=bad)
    for bad in (0, -4, True, 2.5, (16,), (16, 0), (16, 24, 8), "16", None, (16, True)):
        with pytest.raises(ValueError, match="n_sims"):
            e.play(bad)
    for bad in (-1, 1.5, True, "2"):
        with pytest.raises(ValueError, match="explore_turns"):
            e.play(16, explore_turns=bad)
    for bad in (1, 0, "yes"):
        with pytest.raises(ValueError, match="one_launch"):
            e.play(16, one_launch=bad)
    assert e._n_sims(16) == (16, 16) and e._n_sims((16, 24)) == (16, 24) and e._n_sims([100, 400]) == (100, 400)
