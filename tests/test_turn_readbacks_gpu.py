"""The turn loop reads back ONCE per turn (engine.SelfPlayEngine._play_turns: every side's error flags, the checks of the
moves, the end-of-game test and the counts the next searches start from travel in one tolist), whoever drives it:
self-play with its rules off and with all three on, a match, the arena in both forms.  Measured as the difference
between the same configuration played for 8 and for 4 turns -- no Othello game ends before turn 9, so every turn is
played -- of the Tensor.tolist / Tensor.item calls on device tensors: 4, one per added turn, whatever the set-up before
the first turn costs.  Sizes of test_arena_gpu.py: 16 games, 16 playouts, n_thr 2, pools that never compact."""
import pytest
import torch

from tests.conftest import load_json

pytestmark = pytest.mark.gpu

G, N_SIMS, N_THR = 16, 16, 2     # (n_thr 2: at the default 15 no root expands in 16 playouts)


@pytest.fixture(scope="module")
def nets():
    from iago_amd import engine, network, ops
    assert torch.cuda.is_available()
    torch.manual_seed(3)
    g = load_json("simulate.json")
    return engine, network.SLPolicy().cuda().eval(), network.Value().cuda().eval(), ops.RolloutWeights(g["shipped_w"], g["shipped_b"])


def _mcts(nets, k=0):
    engine, policy, value, rw = nets
    return engine.BatchedMCTS(G, policy, value, rw, n_thr=N_THR, capacity=engine.suggest_capacity(N_SIMS, N_THR), seed=11 + k,
                              game_id_base=300 + 1000 * k, persistent=True)


def _selfplay(how):
    def play(nets, T):
        m = _mcts(nets)
        return [m], lambda: nets[0].SelfPlayEngine(m, max_turns=T), how
    return play


def _arena(one_launch):
    def play(nets, T):
        ms = [_mcts(nets, 0), _mcts(nets, 1)]
        return ms, lambda: nets[0].ArenaEngine(*ms, max_turns=T), lambda e: e.play(N_SIMS, one_launch=one_launch)
    return play


CASES = {
    "selfplay": _selfplay(lambda e: e.play(N_SIMS)),
    "selfplay_all_rules": _selfplay(lambda e: e.play(N_SIMS, solve_empties=2, explore_turns=4, playout_cap=(4, 128))),
    "match": _selfplay(lambda e: e.play_match(N_SIMS, mcts_colour=2)),
    "arena_sequential": _arena(False),
    "arena_one_launch": _arena(True),
}


@pytest.mark.parametrize("case", list(CASES))
def test_a_turn_more_is_one_readback_more(nets, case, monkeypatch):
    monkeypatch.setenv("IAGO_PERSISTENT_GAMES", "0")
    calls = []
    for name in ("tolist", "item"):
        def counted(self, *a, _f=getattr(torch.Tensor, name), **k):
            if self.is_cuda:
                calls.append(1)
            return _f(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, counted)
    got = {}
    for T in (4, 8):
        ms, make, play = CASES[case](nets, T)
        e = make()
        del calls[:]
        r = play(e)
        got[T] = len(calls)
        assert r.n_turns == T and all(m.n_compactions == 0 for m in ms)      # (the turn loop, every turn of it)
        if case == "arena_one_launch":
            assert e.n_arena_launches > 0
        for m in ms:
            m.close()
    print("%s: host readbacks in 4 turns %d, in 8 turns %d" % (case, got[4], got[8]))
    assert got[8] - got[4] == 4
