"""The rules of iago_canonical_rows, iago_replay_merge and iago_replay_sample_merged (include/iago_hip_training.h) in
numpy, on tests/replay_ref.py's cell maps and draw.  Everything is in integers but one float32 division, so the
device's outputs are pinned bit for bit.

    canonical   k* = the lowest k in 0 .. 7 whose pair (variant k of own, variant k of opp) is smallest, own compared
                first, then opp, as unsigned 64-bit; (c_own, c_opp) = that pair, sym = k*
    merge       over the slots 0 .. count-1: a group per distinct (c_own, c_opp), numbered in ascending (c_own, c_opp);
                pi[g][m_sym(a)] += pi[slot][a] (the visit row turned into the canonical frame), z_sum[g] += z[slot],
                mult[g] += 1, first = the exclusive prefix sum of mult; sums beyond int32 are stored as the nearest end
                of its range and raise bit 1 of the flags
    draw        row j: replay_ref.draw's Philox words; sym = c[1] & 7; "unique": g = (c[0] * n_unique) >> 32; "rows":
                r = (c[0] * count) >> 32 and g the group with first[g] <= r < first[g] + mult[g]
    row j       variant sym of group g's boards and summed visit row, result = float32(z_sum) / float32(mult)"""
import numpy as np

from tests import replay_ref

OVERFLOW = 2   # the bit of the flags a clamped sum raises
I32 = np.iinfo(np.int32)
_CELLS = np.arange(64, dtype=np.uint64)
_MAPS = [np.array(replay_ref.cell_map(k)) for k in range(8)]


def random_game_rows(games=64, seed=0):
    """The rows of `games` uniformly random games on the oracle's rules, one per turn with a legal move, in game
    order: own / opp (uint64, own = the mover), turn (the row's number within its game), pi (int32, 0 .. 400 on the
    legal cells, 0 elsewhere), z (int8 in -1 .. 1), all drawn from RandomState(seed).  Random games leave the start
    position slowly: groups of `games` rows (turns 0 and 1) and of about a third of that (turn 2) come with them."""
    from oracle import oracle as orc
    rs = np.random.RandomState(seed)
    own, opp, turn, pi = [], [], [], []
    for _ in range(games):
        s, colour, t = orc.initial_state(), 1, 0
        while True:
            acts = orc.legal_actions(s, colour)
            if not acts:
                colour = 3 - colour
                acts = orc.legal_actions(s, colour)
                if not acts:
                    break
            p1, p2 = orc.state_to_bits(s)
            own.append(p1 if colour == 1 else p2)
            opp.append(p2 if colour == 1 else p1)
            turn.append(t)
            row = np.zeros(64, dtype=np.int32)
            row[acts] = rs.randint(0, 401, size=len(acts))
            pi.append(row)
            orc.place_stone(s, acts[rs.randint(len(acts))], colour)
            colour, t = 3 - colour, t + 1
    return dict(own=np.array(own, dtype=np.uint64), opp=np.array(opp, dtype=np.uint64), turn=np.array(turn),
                pi=np.stack(pi), z=rs.randint(-1, 2, size=len(own)).astype(np.int8))


def turn_boards(x, k):
    """Variant k of uint64 boards: bit m_k(a) set where x has bit a set."""
    x = np.asarray(x, dtype=np.uint64).reshape(-1)
    on = (x.reshape(-1, 1) >> _CELLS) & np.uint64(1)
    out = np.zeros_like(on)
    out[:, _MAPS[k]] = on
    return np.bitwise_or.reduce(out << _CELLS, axis=1)


def turn_rows(pi, k):
    """Variant k of (n, 64) visit rows: out[:, m_k(a)] = pi[:, a]."""
    pi = np.asarray(pi).reshape(-1, 64)
    out = np.zeros_like(pi)
    out[:, _MAPS[k]] = pi
    return out


def canonical(own, opp):
    """(c_own, c_opp) uint64 and sym uint8 of the rows (own, opp), given as uint64 arrays."""
    own, opp = np.asarray(own, dtype=np.uint64).reshape(-1), np.asarray(opp, dtype=np.uint64).reshape(-1)
    c_own, c_opp, sym = own.copy(), opp.copy(), np.zeros(own.size, dtype=np.uint8)
    for k in range(1, 8):
        o, p = turn_boards(own, k), turn_boards(opp, k)
        less = (o < c_own) | ((o == c_own) & (p < c_opp))          # (strictly: a tie keeps the lower k)
        c_own, c_opp, sym = np.where(less, o, c_own), np.where(less, p, c_opp), np.where(less, np.uint8(k), sym)
    return c_own, c_opp, sym.astype(np.uint8)


def merge(own, opp, pi, z, count):
    """The window's slots 0 .. count-1 merged: a dict own, opp (uint64), pi (n_unique, 64) int32, z_sum, mult int32,
    first int64, n_unique, flags.  own / opp: uint64 arrays; pi (capacity, 64); z (capacity,)."""
    count = int(count)
    c_own, c_opp, sym = canonical(np.asarray(own)[:count], np.asarray(opp)[:count])
    keys = sorted(set(zip(c_own.tolist(), c_opp.tolist())))        # (Python ints: unsigned, own first)
    number = {key: g for g, key in enumerate(keys)}
    group = np.array([number[key] for key in zip(c_own.tolist(), c_opp.tolist())], dtype=np.int64)
    n_unique = len(keys)
    turned = np.zeros((count, 64), dtype=np.int64)
    for k in range(8):
        at = np.nonzero(sym == k)[0]
        turned[at] = turn_rows(np.asarray(pi)[:count][at].astype(np.int64), k)
    pi_sum = np.zeros((n_unique, 64), dtype=np.int64)
    np.add.at(pi_sum, group, turned)
    z_sum = np.zeros(n_unique, dtype=np.int64)
    np.add.at(z_sum, group, np.asarray(z)[:count].astype(np.int64))
    mult = np.bincount(group, minlength=n_unique).astype(np.int64)
    over = bool(((pi_sum > I32.max) | (pi_sum < I32.min)).any() or ((z_sum > I32.max) | (z_sum < I32.min)).any())
    return dict(own=np.array([key[0] for key in keys], dtype=np.uint64), opp=np.array([key[1] for key in keys], dtype=np.uint64),
                pi=np.clip(pi_sum, I32.min, I32.max).astype(np.int32), z_sum=np.clip(z_sum, I32.min, I32.max).astype(np.int32),
                mult=mult.astype(np.int32), first=(np.cumsum(mult) - mult).astype(np.int64), n_unique=n_unique,
                flags=OVERFLOW if over else 0)


def draw(seed, step, j, mode, first, count):
    """(group, sym) of output row j; first: the merged rows' first (its length is n_unique)."""
    if mode == "unique":
        return replay_ref.draw(seed, step, j, len(first))
    if mode != "rows":
        raise ValueError(mode)
    r, sym = replay_ref.draw(seed, step, j, count)
    return int(np.searchsorted(first, r, side="right")) - 1, sym


def sample(merged, count, seed, step, n, mode):
    """The n output rows of a merged draw: own, opp (uint64), pi int32, result float32, z_sum, mult, group int32, sym
    uint8.  merged: merge()'s dict (or the same columns from elsewhere); count: the window's rows."""
    first = np.asarray(merged["first"], dtype=np.int64)
    draws = np.array([draw(seed, step, j, mode, first, count) for j in range(n)], dtype=np.int64).reshape(n, 2)
    g, sym = draws[:, 0], draws[:, 1]
    out = dict(own=np.zeros(n, np.uint64), opp=np.zeros(n, np.uint64), pi=np.zeros((n, 64), np.int32),
               z_sum=np.asarray(merged["z_sum"], dtype=np.int32)[g], mult=np.asarray(merged["mult"], dtype=np.int32)[g],
               group=g.astype(np.int32), sym=sym.astype(np.uint8))
    for k in range(8):
        at = np.nonzero(sym == k)[0]
        if at.size:
            out["own"][at] = turn_boards(np.asarray(merged["own"], dtype=np.uint64)[g[at]], k)
            out["opp"][at] = turn_boards(np.asarray(merged["opp"], dtype=np.uint64)[g[at]], k)
            out["pi"][at] = turn_rows(np.asarray(merged["pi"], dtype=np.int32)[g[at]], k)
    out["result"] = out["z_sum"].astype(np.float32) / out["mult"].astype(np.float32)
    return out
