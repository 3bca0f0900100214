"""Helpers of the oracle checks of whole-batch launches (tests/test_bench_batch_gpu.py,
tests/test_split_default_sizes_gpu.py) and of their worker processes (tests/rebuild_worker.py): the oracle's policy_fn / value_fn as the production kernels on
ONE board, the rebuild of a recorded game's searches with oracle/mcts_py.MCTS (MCTS.py:105-154), the replay of every
record through the C oracle, the audit of the position table, and the rules check of a match's records.  A batch is a
dict of host arrays (records [T][games], z_log [rows][games], ...); the game count comes from the arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import torch

from oracle import mcts_py
from oracle import oracle as orc
from tests import table_util


def make_nets():
    """bench.mcts_leg's nets, to the letter (random init, seed 0)."""
    from iago_amd import network
    torch.manual_seed(0)
    policy = network.SLPolicy().cuda().eval()
    value = network.Value().cuda().eval()
    value.split_f16 = True
    return policy, value


class Probe(object):
    """policy_fn / value_fn of the oracle: the production kernels on ONE board, memoised."""

    def __init__(self, B):
        self.ops, self.policy, self.value = B["ops"], B["policy"], B["value"]
        self.p_cache, self.v_cache = {}, {}
        self.idx = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.one = torch.ones(1, dtype=torch.int32, device="cuda")
        self.out = torch.zeros(1, dtype=torch.float32, device="cuda")

    def _boards(self, x):
        x = np.asarray(x, np.float32).reshape(2, 64)
        own = sum(1 << a for a in range(64) if x[1, a] == 1.0)   # channel 1 = side to move
        opp = sum(1 << a for a in range(64) if x[0, a] == 1.0)
        return (own, opp), self.ops.bits_to_tensor([own]), self.ops.bits_to_tensor([opp])

    def policy_fn(self, x):
        key, o, p = self._boards(x)
        if key not in self.p_cache:
            self.p_cache[key] = self.policy.forward_boards_split3(o, p).cpu().numpy().reshape(64).copy()
        return self.p_cache[key]

    def value_fn(self, x):
        key, o, p = self._boards(x)
        if key not in self.v_cache:
            with torch.no_grad():
                self.value.forward_boards_counted(o, p, self.idx, self.one, self.out)
            self.v_cache[key] = np.float32(self.out.cpu().numpy()[0])
        return self.v_cache[key]


def rebuild(B, probe, g, n_turns, n_thr=15, compare_from=0, col=None):
    """(ii): game g's first n_turns turns searched again by the oracle's MCTS.py restatement: root visit counts by
    action and moves equal the launch's records (from turn compare_from on: the searches before it are run all the
    same -- MCTS.update_with_move carries the subtree from search to search).  col: g's column in B's arrays (default
    g).  Returns the searches compared."""
    n_sims = B["n_sims"]
    c = g if col is None else col
    it = iter(B["zlog"][:B["zn"][c], c])
    om = mcts_py.MCTS(probe.policy_fn, probe.value_fn, lambda s, c: int(next(it)), lmbda=0.5, c_puct=1.0, n_thr=n_thr)
    state = orc.initial_state()
    stone_num, pass_flg, t, n_cmp = 4, False, 0, 0
    while stone_num < 64 and t < n_turns:
        for color in (1, 2):
            acts = orc.legal_actions(state, color)
            if len(acts) > 0:
                a = om.get_move(state, color, n_sims)
                want = np.zeros(64, np.int64)
                for act, ch in om.root.children.items():
                    want[act] = ch.n_visits
                if t >= compare_from:
                    assert B["pi"][t, c].tolist() == want.tolist(), (g, t)
                    assert int(B["move"][t, c]) == a, (g, t)
                    n_cmp += 1
                om.update_with_move(a)
                orc.place_stone(state, a, color)
                stone_num += 1
                pass_flg = False
            else:
                if pass_flg:
                    stone_num = 64
                pass_flg = True
                om.update_with_move(-1)
            t += 1
            if t >= n_turns:
                break
    if n_turns >= B["game_turns"][c]:
        assert next(it, None) is None, g      # the oracle consumed exactly the playouts the launch ran
    B.setdefault("max_path", {})[g] = om.max_path   # the deepest descent (nodes on a playout's path, the root included)
    return n_cmp




def rebuild_in_workers(B, jobs, tmp_path, n_workers=4):
    """jobs: [(game, turns to rebuild, compare from turn)] spread over worker processes (tests/rebuild_worker.py: the
    Python restatement of MCTS.py with the nets' outputs from the production kernels on one board, each worker its
    own HIP context).  Returns (searches compared, {game: deepest path})."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    procs = []
    for w in range(n_workers):
        mine = jobs[w::n_workers]
        if not mine:
            continue
        arrays = dict(n_sims=B["n_sims"], n_thr=B["n_thr"], games=np.array([j[0] for j in mine]),
                      n_turns=np.array([j[1] for j in mine]), compare_from=np.array([j[2] for j in mine]))
        for g, _, _ in mine:
            arrays["pi_%d" % g], arrays["move_%d" % g] = B["pi"][:, g], B["move"][:, g]
            arrays["zlog_%d" % g] = B["zlog"][:B["zn"][g], g]
            arrays["game_turns_%d" % g] = B["game_turns"][g]
        src, dst = os.path.join(str(tmp_path), "job%d.npz" % w), os.path.join(str(tmp_path), "job%d.json" % w)
        np.savez(src, **arrays)
        procs.append((subprocess.Popen([sys.executable, os.path.join(root, "tests", "rebuild_worker.py"), src, dst], cwd=root), dst))
    n, depth = 0, {}
    for p, dst in procs:
        rc = p.wait(timeout=600)
        out = json.load(open(dst))
        assert rc == 0 and "error" not in out, out.get("error")
        n += sum(out["compared"].values())
        depth.update({int(g): d for g, d in out["max_path"].items()})
    return n, depth


def replay_records(B, whole, games=None):
    """(i): every record of the games (default: all the arrays hold) through the C oracle.  Returns the number of
    records checked."""
    own, opp, valid, move, pi, T, n_sims = B["own"], B["opp"], B["valid"], B["move"], B["pi"], B["T"], B["n_sims"]
    n_rec = 0
    for g in (range(valid.shape[1]) if games is None else games):
        state = orc.initial_state()
        stone_num, pass_flg, t = 4, False, 0
        over = False
        while not over and t < T:
            for color in (1, 2):
                p1, p2 = orc.state_to_bits(state)
                mover = (p1, p2) if color == 1 else (p2, p1)
                assert (int(own[t, g]), int(opp[t, g])) == mover, (g, t)
                acts = orc.legal_actions(state, color)
                if len(acts) > 0:
                    assert valid[t, g] == 1, (g, t)
                    a = int(move[t, g])
                    assert a in acts, (g, t, a)
                    row = pi[t, g]
                    assert np.all(row[[x for x in range(64) if x not in acts]] == 0), (g, t)
                    assert a == int(np.argmax(row)) and row[a] > 0, (g, t)      # first most-visited child (MCTS.py:147)
                    # the root was a leaf for its first visits, then every playout went to a child (MCTS.py:109)
                    assert int(row.sum()) >= n_sims - B["n_thr"], (g, t)   # (+ the visits the reused subtree brought)
                    orc.place_stone(state, a, color)
                    stone_num += 1
                    pass_flg = False
                else:
                    assert valid[t, g] == 0 and move[t, g] == -1 and not pi[t, g].any(), (g, t)
                    if pass_flg:
                        stone_num = 64
                    pass_flg = True
                n_rec += 1
                t += 1
                if t >= T:
                    break
            if stone_num >= 64:
                over = True
        if whole:
            assert over and B["game_turns"][g] == t, (g, t, B["game_turns"][g])
            assert B["z"][g] == orc.judge(state, 1), g
            assert orc.state_to_bits(state) == (int(B["f1"][g]), int(B["f2"][g])), g
        else:
            assert B["game_turns"][g] == T, g
    return n_rec


def audit_table(B, n_walk, n_games=None):
    """(iii): the position table after the batch; every entry's writer is one of the batch's n_games games (default:
    the records' game count)."""
    n_games = B["valid"].shape[1] if n_games is None else n_games
    # (tests/table_util.py: no odd sequence word, value word and sequence word agree, the writers, disjoint stones, every
    # entry in the slot a lookup reads, and n_walk sampled entries against the one-board walk, ONE board per launch)
    n_used, n_walked = table_util.audit(B["table"], B["value"], n_writers=n_games, n_walk=n_walk)
    assert n_used > 1000
    return n_used, n_walked


def replay_match(s, g, n_sims, n_thr=15, on_turn=None):
    """Game g of a match result s (host arrays; SelfPlayEngine.play_match) through the C oracle (game.py:96-145,
    246-262), every record checked; on_turn(t, state, color, kind, acts) is called before each move ('search' / 'draw' /
    'forced' / 'pass').  Returns the game's turns."""
    own, opp = s["own"].view(np.uint64), s["opp"].view(np.uint64)    # (bit 63 set: a negative int64)
    mc = int(s["mcts_colour"][g])
    state = orc.initial_state()
    stone_num, pass_flg, t, over = 4, False, 0, False
    while not over and t < 128:
        for color in (1, 2):
            p1, p2 = orc.state_to_bits(state)
            assert (int(own[t, g]), int(opp[t, g])) == ((p1, p2) if color == 1 else (p2, p1)), (g, t)
            acts = orc.legal_actions(state, color)
            row = s["pi"][t, g]
            a = int(s["move"][t, g])
            if len(acts) > 0:
                kind = "forced" if stone_num > 62 and len(acts) == 1 else ("search" if color == mc else "draw")
                assert a in acts, (g, t, a)
                if kind == "search":
                    assert s["valid"][t, g] == 1, (g, t)
                    assert np.all(row[[x for x in range(64) if x not in acts]] == 0), (g, t)
                    assert a == int(np.argmax(row)) and int(row.sum()) >= n_sims - n_thr, (g, t)
                else:
                    assert s["valid"][t, g] == 2 and not row.any(), (g, t, kind)
                if on_turn:
                    on_turn(t, state, color, kind, acts)
                orc.place_stone(state, a, color)
                stone_num += 1
                pass_flg = False
            else:
                assert s["valid"][t, g] == 0 and a == -1 and not row.any(), (g, t)
                if on_turn:
                    on_turn(t, state, color, "pass", acts)
                if pass_flg:
                    stone_num = 64
                pass_flg = True
            t += 1
        if stone_num >= 64:
            over = True
    assert over and t % 2 == 0 and int(s["game_turns"][g]) == t, (g, t)
    assert s["z"][g] == orc.judge(state, 1), g
    assert orc.state_to_bits(state) == (int(s["final_p1"].view(np.uint64)[g]), int(s["final_p2"].view(np.uint64)[g])), g
    return t
