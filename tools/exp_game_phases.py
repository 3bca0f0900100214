"""Lab tool: where a game workgroup's iteration goes (replies + moves, descent, rollouts, backup, end of iteration), clock
stamps of game workgroup 0.  Needs the stamped variant of the search kernel:

    python tools/build_search_variants.py
    IAGO_HIP_LIB=$PWD/tools/_build/search_phases.so python tools/exp_game_phases.py [playouts] [n_thr] [--from-turn T] [--walk]

--from-turn T: only the iterations in which the workgroup's first game stands at turn T or later are stamped (the end of a
batch, where the pass chains are: 8 empties remain from turn 52 on when nobody has passed); the configurations that end
before turn T are left out.  --walk: the descent walks every level (BatchedMCTS(chain_skip=False)), for the A/B.
"""
import ctypes as C, os, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
from iago_amd import _lib, engine, network, ops
L = _lib.lib()
L.iago_debug_game_phases.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
ARGV, FROM, WALK = [], 0, "--walk" in sys.argv
for i, a in enumerate(sys.argv[1:], 1):
    if a == "--from-turn":
        FROM = int(sys.argv[i + 1])
    elif not a.startswith("--") and sys.argv[i - 1] != "--from-turn":
        ARGV.append(a)
buf = (C.c_ulonglong * 8)()
w, b = bench.shipped_rollout_weights()
NAMES = ("replies + moves", "descent", "control words", "packing + rollout passes", "backup", "end of iteration")
# python tools/exp_game_phases.py [playouts per move = 100] [n_thr = 15]   (round 6: 400 / 15 = configs[3]'s share, 100 / 1)
SIMS = int(ARGV[0]) if len(ARGV) > 0 else 100
N_THR = int(ARGV[1]) if len(ARGV) > 1 else 15
L.iago_debug_game_phases_from(FROM)
for games, turns in ((1024, 128), (1024, 12), (64, 128)):
    if turns <= FROM:
        continue
    torch.manual_seed(0)
    policy, value = network.SLPolicy().cuda().eval(), network.Value().cuda().eval()
    m = engine.BatchedMCTS(games, policy, value, ops.RolloutWeights(w, b), n_thr=N_THR, seed=7, persistent=True, split=0, **(dict(chain_skip=False) if WALK else {}),
                           capacity=engine.suggest_capacity(SIMS, N_THR, moves=64))
    eng = engine.SelfPlayEngine(m, max_turns=turns)
    L.iago_debug_game_phases(buf, 1)
    eng.play(SIMS, record=False)
    torch.cuda.synchronize()
    L.iago_debug_game_phases(buf, 1)
    t = list(buf)
    it = max(1, t[7])
    print("%d playouts per move, n_thr %d; games %d, %d turns%s%s: game workgroup 0: %d iterations, %.1f us each:"
          % (SIMS, N_THR, games, turns, ", from turn %d on" % FROM if FROM else "", ", every level walked" if WALK else "", it,
             sum(t[:6]) / it / 100.0))
    print("   " + ";  ".join("%s %.2f" % (n, x / it / 100.0) for n, x in zip(NAMES, t[:6])))
    if m._ps["totals"].numel() > 16:
        print("   levels of remembered pass chains jumped over (all game workgroups): %d" % int(m._ps["totals"][16].item()))
    m.close()
