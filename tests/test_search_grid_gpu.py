"""The net workgroups every launch form of the persistent search gets (csrc/search_kernel.hip, the host launch layer):
after a launch, ctl word 7 holds what the grid was given beside the game workgroups, and that is
min(net_workgroups, min(max_cus, CUs) x workgroups per CU - game workgroups), CUs and workgroups per CU being
iago_mcts_search_capacity's.  Shapes: the smallest at which the bound bites -- 16 net workgroups asked for, 8 CUs to
count on, two game workgroups -- for the single, the wave, the park and the arena launch (the role split's grid is
pinned by tests/test_split_default_sizes_gpu.py, the single launch's default size by tests/test_search_persistent_gpu.py)."""
import ctypes as C

import pytest
import torch

from tests.bench_batch_util import make_nets
from tests.conftest import load_json

pytestmark = pytest.mark.gpu

N_THR, N_SIMS, NET, MAX_CUS = 2, 16, 16, 8   # (at the default n_thr of 15 no root expands in 16 playouts)


@pytest.fixture(scope="module")
def nets():
    from iago_amd import engine, ops
    assert torch.cuda.is_available()
    policy, value = make_nets()
    g = load_json("simulate.json")
    return engine, ops, policy, value, ops.RolloutWeights(g["shipped_w"], g["shipped_b"])


def _want(game_wgs):
    from iago_amd import _lib
    cus, per = C.c_int32(0), C.c_int32(0)
    assert _lib.lib().iago_mcts_search_capacity(C.byref(cus), C.byref(per)) == 0
    want = min(NET, min(MAX_CUS, cus.value) * per.value - game_wgs)
    assert 1 <= want < NET          # (the bound bites)
    return want


def _engine(nets, monkeypatch, n_games, moves=2, seed=21, **kw):
    """An engine that asks for NET net workgroups on the whole device and is then told to count on MAX_CUS CUs: the
    library, not the engine, cuts the grid down."""
    engine, ops, policy, value, rw = nets
    monkeypatch.setenv("IAGO_PERSISTENT_GPW", "32")
    m = engine.BatchedMCTS(n_games, policy, value, rw, n_thr=N_THR, capacity=engine.suggest_capacity(N_SIMS, N_THR, moves=moves),
                           seed=seed, game_id_base=1000 * seed, persistent=True, net_workgroups=NET, split=0, **kw)
    assert m.persistent and m._split is None and m.games_per_workgroup == 32 and m.net_workgroups == NET
    m.max_cus = MAX_CUS
    return m


def _launched(m):
    torch.cuda.synchronize()
    ctl = m._ps["ctl"].tolist()
    assert ctl[3] == 0              # (it did not give up)
    return ctl[7]


def _roots(nets, n):
    engine, ops = nets[0], nets[1]
    own = torch.full((n,), engine.START_OWN, dtype=torch.int64, device="cuda")
    opp = torch.full((n,), engine.START_OPP, dtype=torch.int64, device="cuda")
    return own, opp, torch.ones(n, dtype=torch.uint8, device="cuda")


def test_single(nets, monkeypatch):
    m = _engine(nets, monkeypatch, 64)
    m.search(*_roots(nets, 64), N_SIMS)
    assert _launched(m) == _want(2)
    m.close()


def test_wave(nets, monkeypatch):
    m = _engine(nets, monkeypatch, 8, wave=8)
    assert m.wave_entry
    m.search(*_roots(nets, 8), N_SIMS)
    assert _launched(m) == _want(2)
    m.close()


def test_park(nets, monkeypatch):
    """64 whole games that hand over at 20 empties (the launch alone: nobody plays the parked games out here)."""
    engine = nets[0]
    m = _engine(nets, monkeypatch, 64, moves=64)
    eng = engine.SelfPlayEngine(m)
    own, opp = eng._start_boards(64)
    rec = eng._new_records(64)
    game = dict(max_turns=eng.max_turns, games_total=0, own=own, opp=opp,
                n_turns=torch.zeros(64, dtype=torch.int32, device="cuda"), **{"rec_" + k: v for k, v in rec.items()})
    park = dict(parked=torch.zeros(64, dtype=torch.uint8, device="cuda"), stones=torch.zeros(64, dtype=torch.int32, device="cuda"),
                pass_flg=torch.zeros(64, dtype=torch.uint8, device="cuda"))
    m.tree.reset()
    m._forget_stale_values()
    m._launch_persistent(None, None, torch.ones(64, dtype=torch.uint8, device="cuda"), N_SIMS,
                         engine._play_rules(N_SIMS, solve_empties=20), game=game, park=park)
    assert _launched(m) == _want(2)
    assert int(park["parked"].sum().item()) > 0      # (the park kernel ran: games were handed over)
    m.close()


def test_arena(nets, monkeypatch):
    """32 + 32 games: one game workgroup per agent, max_cus in both sets; the per-CU figure is the arena kernel's own,
    which on this device is the search kernel's."""
    ops = nets[1]
    ms = [_engine(nets, monkeypatch, 32, seed=21 + i) for i in range(2)]
    args, keep = [], []
    for m in ms:
        m._forget_stale_values()
        m.reserve_net_rows(2 + NET)
        a, k = m._search_args(*_roots(nets, 32), N_SIMS)
        assert a.max_cus == MAX_CUS and a.net_workgroups == NET
        args.append(a)
        keep.append(k)
    ops.search_arena(args[0], args[1])
    assert _launched(ms[0]) == _launched(ms[1]) == _want(2)
    del keep
    for m in ms:
        m.close()
