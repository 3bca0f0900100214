#!/usr/bin/env python3
"""The loss against perfect play of PV-MCTS with the shipped nets: how many discs each searched move gives away in the
last empties (engine.endgame_errors: the exact value of every move, ops.solve_endgame_moves(moves="all")).

    python tools/run_endgame_errors.py [--games 1024] [--sims 100,400] [--max-empties 8,10] [--explore-turns 8]
                                       [--out profiles/endgame_errors.json]

Per backup rule x selection rule x playouts: `--games` games of PV-MCTS self-play (explore_turns, no solve_empties), then
endgame_errors over the searched rows (valid == 1) at each max_empties -- rows, skipped, mean_loss (discs per move),
optimal_rate, blunder_rate (the sign of the value changed) -- and the same figures for the raw SLPolicy argmax (the
legal move of the highest probability) on the same positions.  One JSON line per run; --out: all of them as a list."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIGURES = ("rows", "skipped", "mean_loss", "optimal_rate", "blunder_rate")


def policy_argmax(policy, own, opp):
    """(n,) int8: the legal move of the highest SLPolicy probability at every position (own = the mover)."""
    from iago_amd import ops
    cells = torch.arange(64, device=own.device)
    out = []
    with torch.no_grad():
        for at in range(0, own.numel(), 4096):
            o, p = own[at:at + 4096].contiguous(), opp[at:at + 4096].contiguous()
            probs = policy(ops.encode_planes(o, p)).reshape(-1, 64).float()
            legal = ((ops.legal_moves(o, p).reshape(-1, 1) >> cells) & 1).bool()
            out.append(torch.where(legal, probs, torch.full_like(probs, float("-inf"))).argmax(dim=1).to(torch.int8))
    return torch.cat(out) if out else torch.zeros(0, dtype=torch.int8, device=own.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--sims", default="100,400")
    ap.add_argument("--max-empties", default="8,10")
    ap.add_argument("--explore-turns", type=int, default=8)
    ap.add_argument("--n-thr", type=int, default=15)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from iago_amd import engine, network, ops
    policy = network.SLPolicy().load_npz(os.path.join(GOLDEN, "sl_model.npz")).cuda().eval()
    value = network.Value().load_npz(os.path.join(GOLDEN, "value_model.npz")).cuda().eval()
    rollout = network.RolloutPolicy().load_npz(os.path.join(GOLDEN, "rollout_model.npz")).eval()
    rw = ops.RolloutWeights(*rollout.kernel_weights())
    ints = lambda s: [int(x) for x in s.split(",") if x]   # noqa: E731
    lines = []
    for backup in ("reference", "negamax"):
        for selection in ("reference", "alphazero"):
            for sims in ints(args.sims):
                m = engine.BatchedMCTS(args.games, policy, value, rw, lmbda=0.5, c_puct=1.0, n_thr=args.n_thr, seed=args.seed,
                                       persistent=True, backup=backup, selection=selection,
                                       capacity=engine.suggest_capacity(sims, args.n_thr, moves=64))
                res = engine.SelfPlayEngine(m).play(sims, explore_turns=args.explore_turns or None)
                t = res.tuples()
                own, opp, move = t["own"].contiguous(), t["opp"].contiguous(), t["move"]
                raw = policy_argmax(policy, own, opp)
                row = dict(tool="run_endgame_errors", games=args.games, n_sims=sims, backup=backup, selection=selection,
                           explore_turns=args.explore_turns, n_thr=args.n_thr, seed=args.seed, searched_rows=int(own.numel()))
                for k in ints(args.max_empties):
                    for who, mv in (("pv_mcts", move), ("slpolicy_argmax", raw)):
                        e = engine.endgame_errors(own, opp, mv, max_empties=k)
                        row["%s_at_%d" % (who, k)] = {f: e[f] for f in FIGURES}
                m.close()
                lines.append(row)
                print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("[\n" + ",\n".join(json.dumps(x, sort_keys=True) for x in lines) + "\n]\n")


if __name__ == "__main__":
    main()
