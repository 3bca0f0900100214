#!/usr/bin/env python3
"""The PV-MCTS training loop on a replay window: per round one exploring self-play (`games` lockstep games played to
the end, `sims` playouts per move, explore_turns = 8, the learner as the search's policy net, the Value net it
trains as the search's value net, shipped RolloutPolicy) -> ReinforceTrainer.add_to_window (a window of
`window_rounds` rounds' rows) -> `updates_per_round` times one ReplayWindow.sample of `rows` rows (with replacement,
every row in a drawn board symmetry), each feeding BOTH the visit-count update of SLPolicy (_update_visits) and one
native minibatch of the Value net on the rows' results (SupervisedTrainer.step_rows).  One JSON line.
arena_every = k > 0: every k rounds the current nets play `games` arena games (engine.ArenaEngine, `sims` playouts a side)
against a frozen copy of the nets of k rounds ago, and the scores (the current nets' side) join the JSON line.
cap_fast = n > 0: playout-cap randomisation, playout_cap = (n, cap_full) -- a quarter of the turns full by default; the
window still receives tuples() only, the full turns' rows.
noise_eps = e > 0: root noise, root_noise = (noise_alpha, e) in 256ths (alpha 77 / 256 = 0.3, eps 64 / 256 = 0.25 are
the usual setting) -- off by default; such rounds play through the turn loop.
forced_k = k > 0 (with noise_eps > 0): forced playouts and policy-target pruning, forced_playouts = k in 256ths (512 is
KataGo's k = 2) -- the window then receives the PRUNED visit rows; 0 = off.
backup = 1: the negamax backup rule (engine.BatchedMCTS(backup="negamax")) in self-play and on both sides of the gate;
0, the default: the reference's rule.
yardstick_every = k > 0: every k rounds the current nets play `games` games (paired, 8 random opening turns, `sims`
playouts a move) against the fixed-depth alpha-beta opponent of depth yardstick_depth (SelfPlayEngine.play_match(opponent=
engine.AlphaBeta(d))), the one opponent that owes nothing to the nets, and the scores join the JSON line; 0 = off.
selection = 1: the AlphaZero selection rule (engine.BatchedMCTS(selection="alphazero")) in self-play, on both sides of
the gate and against the yardstick; 0, the default: the reference's rule.
solve_empties = k > 0: self-play hands the last k empties to the exact endgame solver (SelfPlayEngine.play(solve_empties=k));
0, the default: off.  solved_targets = 1 (with solve_empties > 0): the solved turns record the set of their optimal moves
(play(solved_targets=True)) and solved_tuples() -- pi 1 on every optimal move -- joins the window beside tuples(); the
JSON line says so and counts those rows.
merge = 1 or 2: the minibatches are drawn out of the window merged by position up to symmetry (ReplayWindow.sample(merged=
"unique") for 1, "rows" for 2): a position's visit rows summed, its results averaged; "unique" draws uniformly over the
distinct positions, "rows" keeps every position's weight in the window and changes the targets only.  0, the default:
every row a position of its own (the JSON line's merge is null).  window_unique, the distinct positions of the window
at the end, is logged beside window_count either way.
gumbel = m > 0 (with backup = 1 and selection = 1, without noise_eps and forced_k: the engine refuses anything else): the
Gumbel root search in self-play, SelfPlayEngine.play(gumbel=(m, 256)) -- fresh roots, sequential halving over the top m
moves, the survivor played, the window receives the improved-policy rows.  The self-play engine then expands at the first
visit (n_thr = 1: at n_thr 15 a budget of 20 would leave the rule five playouts) and no opening moves are drawn from the
visit counts (the rule explores by its own draw); 0, the default: off.
td_lambda = l, q_mix = m, both in 256ths (with backup = 1: a root's Q is a value only under the negamax rule, anything else
is refused): the Value net's labels are the search's own values instead of the game's result alone -- self-play records every
searched root's value (SelfPlayEngine.play(root_values=True)), the rows enter a window with value targets
(ReplayWindow(value_targets=True)) as tuples(value_target=(l, m)) -- TD(lambda) returns along the game with lambda = l / 256,
mixed with m / 256 of the row's own root value (include/iago_hip_training.h, iago_value_targets) -- and step_rows takes the
window's `result`, the target as a float.  256 / 0, the default: the result z, today's loop, which records nothing more.
    python3 tools/run_az_loop.py [iters=100] [games=64] [sims=20] [window_rounds=8] [updates_per_round=4] [rows=1024]
                                 [arena_every=0] [cap_fast=0] [cap_full=64] [noise_eps=0] [noise_alpha=77]
                                 [forced_k=0] [backup=0] [yardstick_every=0] [yardstick_depth=2] [selection=0]
                                 [solve_empties=0] [solved_targets=0] [merge=0] [gumbel=0] [td_lambda=256] [q_mix=0]"""
import copy, json, os, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from iago_amd import engine, network, ops  # noqa: E402
from iago_amd.replay import ReplayWindow  # noqa: E402
from iago_amd.train_rl import ReinforceTrainer  # noqa: E402
from iago_amd.train_supervised import SupervisedTrainer  # noqa: E402

arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d  # noqa: E731
iters, games, sims, window_rounds, updates, rows = arg(1, 100), arg(2, 64), arg(3, 20), arg(4, 8), arg(5, 4), arg(6, 1024)
arena_every = arg(7, 0)
playout_cap = (arg(8, 0), arg(9, 64)) if arg(8, 0) > 0 else None
root_noise = (arg(11, 77), arg(10, 0)) if arg(10, 0) > 0 else None
forced_playouts = arg(12, 0) if arg(12, 0) > 0 else None
backup = engine.backup_arg("negamax" if arg(13, 0) else "reference")
yardstick_every, yardstick_depth = arg(14, 0), arg(15, 2)
selection = engine.selection_arg("alphazero" if arg(16, 0) else "reference")
solve_empties = arg(17, 0) if arg(17, 0) > 0 else None
solved_targets = bool(arg(18, 0))
merge = (None, "unique", "rows")[arg(19, 0)]
gumbel = (arg(20, 0), 256) if arg(20, 0) > 0 else None
td_lambda, q_mix = ops.value_rate_arg(arg(21, 256), "td_lambda"), ops.value_rate_arg(arg(22, 0), "q_mix")
value_target = (td_lambda, q_mix) if (td_lambda, q_mix) != (256, 0) else None
if value_target is not None and backup != "negamax":
    raise ValueError("td_lambda / q_mix need backup = 1 (under the reference's backup rule a root's Q mixes both players' "
                     "views and is no value)")
sp_n_thr = 1 if gumbel is not None else 15
w, b = bench.shipped_rollout_weights()
torch.manual_seed(0)
tr = ReinforceTrainer(network.SLPolicy(), pool_dir=None, N=32, seed=0)
vt = SupervisedTrainer(network.Value(), "value", seed=0, native=True)
m = engine.BatchedMCTS(games, tr.model1, vt.model, ops.RolloutWeights(w, b), n_thr=sp_n_thr,
                       capacity=engine.suggest_capacity(sims, sp_n_thr), seed=1, backup=backup,
                       selection=selection)   # default engine: the persistent search
sp = engine.SelfPlayEngine(m)
window = ReplayWindow(window_rounds * games * 60, seed=2,   # (a game has at most 60 searched turns)
                      value_targets=value_target is not None)
kls, vlosses = [], []
solved_rows = [0]
arena_scores = []
if arena_every > 0:
    # the nets of k rounds ago: a frozen module pair of its own, an engine and tree pool of its own (other seed and ids)
    old_p, old_v = copy.deepcopy(tr.model1).eval(), copy.deepcopy(vt.model).eval()
    m_now = engine.BatchedMCTS(games, tr.model1, vt.model, ops.RolloutWeights(w, b), n_thr=15,
                               capacity=engine.suggest_capacity(sims, 15), seed=3, backup=backup,
                               selection=selection)
    m_old = engine.BatchedMCTS(games, old_p, old_v, ops.RolloutWeights(w, b), n_thr=15,
                               capacity=engine.suggest_capacity(sims, 15), seed=4, game_id_base=games, backup=backup,
                               selection=selection)
    arena = engine.ArenaEngine(m_now, m_old)
yardstick_scores = []
if yardstick_every > 0:
    # an engine and tree pool of its own on the CURRENT nets (other seed and ids), against engine.AlphaBeta
    m_yard = engine.BatchedMCTS(games, tr.model1, vt.model, ops.RolloutWeights(w, b), n_thr=15,
                                capacity=engine.suggest_capacity(sims, 15), seed=5, game_id_base=2 * games, backup=backup,
                                selection=selection)
    yard = engine.SelfPlayEngine(m_yard)
    opponent = engine.AlphaBeta(yardstick_depth)


def yardstick(i):
    """After round i + 1: the current nets against the fixed opponent."""
    tr.model1.eval()
    vt.model.eval()
    s = yard.play_match(sims, opponent=opponent, opening_turns=8, paired=games % 2 == 0, record=False).score()
    yardstick_scores.append(dict(round=i + 1, **s))


def gate(i):
    """After round i + 1: the current nets against the frozen ones, then the frozen ones take the current weights."""
    tr.model1.eval()
    vt.model.eval()
    s = arena.play(sims, record=False).score()
    arena_scores.append(dict(round=i + 1, **s))
    with torch.no_grad():
        for old, new in ((old_p, tr.model1), (old_v, vt.model)):
            for q, p in zip(old.parameters(), new.parameters()):
                q.copy_(p)


def one():
    tr.model1.eval()
    vt.model.eval()
    extra = {} if solve_empties is None else dict(solve_empties=solve_empties, solved_targets=solved_targets)
    if gumbel is not None:
        extra["gumbel"] = gumbel
    if value_target is not None:
        extra["root_values"] = True
    res = sp.play(sims, explore_turns=None if gumbel is not None else 8, playout_cap=playout_cap, root_noise=root_noise,
                  forced_playouts=forced_playouts, **extra)
    added = tr.add_to_window(window, res.tuples(value_target=value_target))
    if solved_targets:
        n = tr.add_to_window(window, res.solved_tuples(value_target=value_target))
        solved_rows[0] += n
        added += n
    for _ in range(updates):
        s = window.sample(rows, merged=merge)   # (merged: the first draw of a round rebuilds the window's snapshot)
        loss = float(tr._update_visits(s["own"], s["opp"], s["pi"]).item())
        kls.append(tr._visits_kl(loss, s["pi"]))
        vlosses.append(vt.step_rows(s["own"], s["opp"], s["result"]))
    return added


for _ in range(2):
    one()
torch.cuda.synchronize()
first = len(kls)
solved_rows[0] = 0   # (the two warm-up rounds are not counted)
t0 = time.perf_counter()
added = 0
for i in range(iters):
    added += one()
    if arena_every > 0 and (i + 1) % arena_every == 0:
        gate(i)
    if yardstick_every > 0 and (i + 1) % yardstick_every == 0:
        yardstick(i)
    if (i + 1) % 25 == 0:
        print("round %d, %.1f s" % (i + 1, time.perf_counter() - t0), file=sys.stderr, flush=True)
torch.cuda.synchronize()
dt = time.perf_counter() - t0
print(json.dumps({"config": "exploring PV-MCTS self-play (%d games per round, %d playouts per move, %s) -> "
                            "replay window of %d rows -> %d x (sample %d rows in random symmetries -> SLPolicy on the "
                            "%s + Value on the results, native), 1 x MI355X"
                            % (games, sims, "explore_turns 8" if gumbel is None else "the Gumbel root search, m %d" % gumbel[0],
                               window.capacity, updates, rows, "visit counts" if gumbel is None else "improved policy"),
                  "rounds": iters, "seconds": dt, "rounds_per_sec": iters / dt,
                  "rows_added": added, "rows_added_per_sec": added / dt,
                  "rows_trained": iters * updates * rows, "rows_trained_per_sec": iters * updates * rows / dt,
                  "window_count": window.count, "window_unique": window.merged().n_unique, "window_total": window.total,
                  "merge": merge,
                  "kl_first": kls[first], "kl_last": kls[-1],
                  "value_loss_first": vlosses[first], "value_loss_last": vlosses[-1],
                  "adam_t_policy": int(tr.opt.t), "adam_t_value": int(vt.opt.t), "playout_cap": playout_cap,
                  "root_noise": root_noise, "forced_playouts": forced_playouts, "gumbel": gumbel, "self_play_n_thr": sp_n_thr, "backup": backup, "selection": selection,
                  "solve_empties": solve_empties, "solved_targets": solved_targets,
                  "td_lambda": td_lambda, "q_mix": q_mix,
                  **({"solved_rows_added": solved_rows[0]} if solved_targets else {}),
                  **({"arena_every": arena_every, "arena": arena_scores} if arena_every > 0 else {}),
                  **({"yardstick_every": yardstick_every, "yardstick_depth": yardstick_depth,
                      "yardstick": yardstick_scores} if yardstick_every > 0 else {})}))
