"""`nodes`, score and move of every lane-per-position search on the device against the restatement of their visiting
order (tests/lane_search_ref.py): the yardstick at depths 1 to 4, the solver exact and wld in launches of 1, 63, 64 and
65, the job lanes of the split search, and the play-out's rows turn by turn.  The other tests hold (score, move) to the
value references and `nodes` only to itself across launches; `nodes` is what shows the order the tree is visited in."""
import numpy as np
import pytest
import torch

from iago_amd import ops

from . import endgame_play_ref as play_ref
from . import endgame_ref as er
from . import lane_search_ref as ls
from .test_alphabeta_gpu import positions  # noqa: F401  (the 64 positions of that test)

pytestmark = pytest.mark.gpu


def _np(r):
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}


def _rows(r, idx=None, prefix=""):
    cols = [r[prefix + k].tolist() for k in ("score", "move", "nodes")]
    rows = list(zip(*cols))
    return rows if idx is None else [rows[i] for i in idx]


@pytest.fixture(scope="module")
def late():
    """64 positions of 2 to 10 empties, roots that must pass among them."""
    own, opp = er.late_positions(64, 29, 2, 10)
    own, opp = [int(a) for a in own], [int(b) for b in opp]
    assert any(not er.bit_legal(a, b) for a, b in zip(own, opp))
    return own, opp


@pytest.fixture(scope="module")
def late_want(late):
    """wld -> [(score, move, nodes)] of the restatement, computed once."""
    own, opp = late
    return {wld: [ls.solve(a, b, wld) for a, b in zip(own, opp)] for wld in (False, True)}


@pytest.mark.parametrize("depth", [1, 2, 3, 4])
def test_yardstick_nodes(positions, depth):  # noqa: F811
    own, opp = positions
    r = _np(ops.alphabeta_moves(ops.bits_to_tensor(own), ops.bits_to_tensor(opp), depth))
    assert r["done"].all()
    assert _rows(r) == [ls.alphabeta(a, b, depth) for a, b in zip(own, opp)]


@pytest.mark.parametrize("mode", ["exact", "wld"])
@pytest.mark.parametrize("n", [64, 1, 63, 65])
def test_solver_nodes(late, late_want, mode, n):
    own, opp = late
    idx = [(5 * i + 2) % 64 for i in range(n)] if n != 64 else list(range(64))
    r = _np(ops.solve_endgame(ops.bits_to_tensor([own[i] for i in idx]), ops.bits_to_tensor([opp[i] for i in idx]),
                              mode=mode, max_empties=10))
    assert r["solved"].all() and r["ctl"][1] >= n
    assert _rows(r) == [late_want[mode == "wld"][i] for i in idx]


@pytest.mark.parametrize("split", [1, 2])
def test_split_job_nodes(positions, split):  # noqa: F811
    own, opp = positions
    r = _np(ops.alphabeta_moves(ops.bits_to_tensor(own), ops.bits_to_tensor(opp), 4, split=split))
    assert r["done"].all() and r["job_done"].all() and r["jobs"] == len(r["job_own"]) > 64
    j_own, j_opp = r["job_own"].view(np.uint64).tolist(), r["job_opp"].view(np.uint64).tolist()
    left = r["job_path"][:, 0].tolist()
    assert min(left) == 4 - split and max(left) == 4    # (depth 4 left: a root that must pass, or a finished game)
    assert _rows(r, prefix="job_") == [ls.alphabeta(a, b, d) for a, b, d in zip(j_own, j_opp, left)]
    # the roots' answer is the unsplit search's
    want = [ls.alphabeta(a, b, 4)[:2] for a, b in zip(own, opp)]
    assert list(zip(r["score"].tolist(), r["move"].tolist())) == want


def test_play_endgame_rows():
    """8 games parked at 8 empties: every turn's (move, score) is the restatement's for that turn's position."""
    own, opp = er.late_positions(8, 31, 8, 8)
    n, T = 8, 128
    games = [(int(a), int(b), 52, 56, 0, T) for a, b in zip(own, opp)]
    want = [play_ref.play_out(*g, solve=lambda a, b: ls.solve(a, b)[:2]) for g in games]
    out = ops.play_endgame(ops.bits_to_tensor([g[0] for g in games]), ops.bits_to_tensor([g[1] for g in games]),
                           torch.full((n,), 52, dtype=torch.int32, device="cuda"),
                           torch.full((n,), 56, dtype=torch.int32, device="cuda"),
                           torch.zeros(n, dtype=torch.uint8, device="cuda"), max_turns=T, max_empties=8)
    torch.cuda.synchronize()
    r_own, r_opp = ops.tensor_to_bits(out["own"]), ops.tensor_to_bits(out["opp"])
    r_valid, r_move, r_score = (out[k].cpu().numpy() for k in ("valid", "move", "score"))
    solved = 0
    for g, w in enumerate(want):
        for t, a, b, valid, move, score in w["rows"]:
            got = (int(r_own[t, g]), int(r_opp[t, g]), int(r_valid[t, g]), int(r_move[t, g]), int(r_score[t, g]))
            assert got == (a, b, valid, move, score), (g, t)
            solved += valid == 3
    assert out["finished"].all() and solved >= 8 * 6
