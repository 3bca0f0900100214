"""MCTS: the reference's search object (MCTS.py:78-154) -- same constructor
arguments, get_move(state, color) and update_with_move(move) -- as a B = 1 view
of the batched HIP engine (engine.BatchedMCTS).

Differences, both forced: the budget is `n_sims` playouts per move when given
(the reference's 10 s wall clock, MCTS.py:142, is kept as the fallback), and
the nets are passed in instead of being read from './models' (MCTS.py:82-85).

wave = W > 1 (8, 16 or 32): the wave search -- W playouts of the tree in flight at once, steered by virtual visits
(virtual_loss per in-flight visit), deterministic (engine.BatchedMCTS, include/iago_hip_serving.h).  W = 1 is the
reference's one-playout-at-a-time order.

solve_empties = k: at a root with at most k empties get_move plays the exact endgame solver's move (the lowest-indexed
move of the best final disc difference, engine.solve_endgame) and runs no search; n_solved counts these moves.  None,
the default, always searches.

backup = "reference" (the default: the reference's update_recursive, the same value at every level) or "negamax" (the
sign turns at every level: engine.backup_arg; the persistent search only, with or without wave=).

selection = "reference" (the default: the reference's Node.select, priors prob + 0.1 and 0.01 + n under the exploration
term) or "alphazero" (priors prob, 1 + n: engine.selection_arg; the persistent search only, with or without wave=).

gumbel = (m, c_scale_256[, c_visit]) (None, the default: off): get_move runs the Gumbel root search (engine.BatchedMCTS.search(
gumbel=); include/iago_hip_serving.h) -- a fresh root, n_sims playouts in sequential halving over the top m moves by
Gumbel + logit, the survivor for a move.  It needs n_sims (the schedule is the budget's), backup="negamax",
selection="alphazero" and wave=1; the k-th get_move of the object draws as turn k of game `seed`'s id 0.
"""
import time

import numpy as np
import torch

from . import boards, engine, ops

SOLVE_EMPTIES_MAX = 20   # what the solver takes (include/iago_hip_serving.h)


def solve_split_depth(empties):
    """The root split of a single-position solve at `empties` empties: the fastest measured on MI355X (LABNOTES
    "Exact endgame")."""
    return 0 if empties <= 8 else (4 if empties <= 10 else 3)


class MCTS(object):

    def __init__(self, lmbda=0.5, c_puct=1, n_thr=15, time_limit=10, policy_net=None,
                 value_net=None, rollout_weights=None, n_sims=None, capacity=65536, seed=0,
                 use_graph=False, wave=1, virtual_loss=1.0, solve_empties=None, backup="reference",
                 selection="reference", gumbel=None):
        if policy_net is None or (value_net is None and lmbda < 1):
            raise ValueError("policy_net / value_net are required (the reference loads "
                             "./models/sl_model.npz and ./models/value_model.npz here)")
        self.lmbda, self.c_puct, self.n_thr, self.time_limit = lmbda, c_puct, n_thr, time_limit
        self.n_sims = n_sims
        self.policy_net, self.value_net = policy_net, value_net
        self._m = engine.BatchedMCTS(1, policy_net, value_net, rollout_weights, lmbda=lmbda,
                                     c_puct=c_puct, n_thr=n_thr, capacity=capacity, seed=seed,
                                     use_graph=use_graph, wave=wave, virtual_loss=virtual_loss, backup=backup,
                                     selection=selection)
        self.wave, self.backup, self.selection = wave, self._m.backup, self._m.selection
        self.chunk = max(8, 4 * wave)   # playouts per search of the time-limited loop
        self._one = torch.ones(1, dtype=torch.uint8, device="cuda")
        if solve_empties is not None and (isinstance(solve_empties, bool) or not isinstance(solve_empties, int) or
                                          not 0 <= solve_empties <= SOLVE_EMPTIES_MAX):
            raise ValueError("solve_empties must be None or an int in [0, %d], got %r" % (SOLVE_EMPTIES_MAX,
                                                                                        solve_empties))
        self.solve_empties = solve_empties
        self.n_solved = 0
        self._root = engine.root_rule(None, gumbel=gumbel, engine=self._m)   # (the turn loop's rule; n_sims: search() checks it)
        self.gumbel = self._root and self._root.gumbel
        if self._root is not None and n_sims is None:
            raise ValueError("gumbel needs n_sims: the halving's schedule is built for the budget")
        self._turn = 0   # (gumbel: searched get_move calls so far, the draw's turn)

    def get_move(self, state, color):
        """MCTS.py:139-147: playouts from the root, then the most visited child."""
        own, opp = boards.own_opp(state, color)
        if self.solve_empties is not None:
            empties = int(np.count_nonzero(np.asarray(state) == 0))
            if empties <= self.solve_empties:
                move = int(engine.solve_endgame(own, opp, split_depth=solve_split_depth(empties))["move"][0].item())
                if move >= 0:   # (a pass or a finished game: the search answers as it always has)
                    self.n_solved += 1
                    return move
        if self._root is not None:   # (the rule's search of turn k, then its move in the engine's move buffer)
            self._m.search(own, opp, self._one, self.n_sims, **self._root._asdict(), turn=self._turn)
            self._turn += 1
            self._root.move(self._m, self._one)
            move = int(self._m.move[0].item())
        else:
            if self.n_sims is not None:
                self._m.search(own, opp, self._one, self.n_sims)
            else:
                start = time.time()
                while time.time() - start < self.time_limit:
                    self._m.search(own, opp, self._one, self.chunk)
            move = int(self._m.best_move(self._one)[0].item())
        if move == -2:   # (what MCTS.py:147 raises)
            raise ValueError("max() arg is an empty sequence: the root has no children (fewer than n_thr playouts)")
        return move

    def update_with_move(self, last_move):
        """MCTS.py:149-154."""
        self._m.update_with_move(torch.tensor([last_move], dtype=torch.int8, device="cuda"))

    @property
    def n_leaf_evals(self):
        return self._m.n_leaf_evals
