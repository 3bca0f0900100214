"""The value targets' rules restated in numpy, from the contracts in include/iago_hip_serving.h (iago_mcts_root_value) and
include/iago_hip_training.h (iago_value_targets, iago_replay_merge_values) -- not from the kernels.  Python integers and
int64 throughout: the GPU must agree bit for bit."""
import numpy as np

Q16 = 65536
ROOT_LIMIT = 1 << 30
SATURATED, NAN = 1, 2      # bits of iago_mcts_root_value's flags
SEARCHED = (1, 4)          # valid of a searched row (a full turn, a fast turn of the playout cap)
SOLVED = 3                 # valid of a row the endgame solver played


def root_value_q16(q, with_flags=False):
    """q: the roots' stored Q (float32; under the negamax rule the value for the player who moved INTO the root).  The
    mover's value in Q16: rint(-q * 65536) -- one float32 multiply, exact, then to nearest, ties to even -- saturated to
    +-2^30; NaN gives 0.  Nothing is clipped at +-65536.  with_flags: also the flags word the values raise."""
    q = np.asarray(q, np.float32)
    out = np.zeros(q.shape, np.int32)
    flags = 0
    for i, x in np.ndenumerate(q):
        if np.isnan(x):
            flags |= NAN
            continue
        with np.errstate(over="ignore"):
            m = np.float32(-x) * np.float32(Q16)      # (a power of two: exact, or infinite)
        if np.isinf(m):
            r = ROOT_LIMIT + 1 if m > 0 else -ROOT_LIMIT - 1
        else:
            r = int(np.rint(np.float64(m)))           # (a float32 is a float64: the same ties, to even)
        if abs(r) > ROOT_LIMIT:
            flags |= SATURATED
            r = ROOT_LIMIT if r > 0 else -ROOT_LIMIT
        out[i] = r
    return (out, flags) if with_flags else out


def value_targets(valid, q, score, z, mover, lam, mix):
    """(T, B) int32: the targets from the mover's view, 0 where there is no row.  The rule is stated in colour 1's frame."""
    valid, q, score = np.asarray(valid), np.asarray(q), np.asarray(score)
    T, B = valid.shape
    assert 0 <= lam <= 256 and 0 <= mix <= 256
    out = np.zeros((T, B), np.int32)
    for b in range(B):
        g_next = v_next = Q16 * int(z[b])
        for t in range(T - 1, -1, -1):
            s = 1 if int(mover[t]) == 1 else -1
            kind = int(valid[t, b])
            if kind in SEARCHED:
                v = s * max(-Q16, min(Q16, int(q[t, b])))
            elif kind == SOLVED:
                sc = int(score[t, b])
                v = s * Q16 * ((sc > 0) - (sc < 0))
            else:
                continue
            g = ((256 - lam) * v_next + lam * g_next + 128) >> 8      # (python's >> floors, as an arithmetic shift)
            r = ((256 - mix) * g + mix * v + 128) >> 8
            out[t, b] = s * r
            g_next, v_next = g, v
    return out


def merge_values(order, group, v):
    """v_sum[g] (int64) = the sum of v[order[i]] over the sorted rows i with group[i] == g."""
    order, group = np.asarray(order, np.int64), np.asarray(group, np.int64)
    out = np.zeros(int(group.max()) + 1, np.int64)
    np.add.at(out, group, np.asarray(v, np.int64)[order])
    return out
