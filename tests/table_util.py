"""What the tests know about the persistent search's position table (iago_mcts_search_args.vtable, include/iago_hip.h;
iago_amd/csrc/search_kernel.hip: vtable_slot, vtable_get, vtable_put_begin, vtable_put_end; the engine's m._vtable).

An entry is four uint64 words:

  [0] the sequence word: high half = the writer (the slot of the game whose request put the value there), low half = the
      sequence number -- 0: never used, odd: being written, even: published;
  [1] own, [2] opp: the position, own = the side to move;
  [3] the value word: high half = the sequence number the value belongs to, low half = the float32's bits.

A lookup accepts an entry whose sequence word is non-zero, even and the same before and after the other three loads,
whose own and opp are the position asked for, and whose value word carries the sequence word's number.  The table is
direct-mapped: the entry of a position lives in slot_of(own, opp, slots - 1) and nowhere else."""
import numpy as np
import torch

LOW = np.uint64(0xFFFFFFFF)


def slot_of(own, opp, mask):
    """vtable_slot restated: 64-bit wrapping arithmetic.  own, opp: Python ints or uint64 arrays; mask = slots - 1.
    Returns an int for ints, an int64 array for arrays."""
    scalar = np.ndim(own) == 0
    o = np.atleast_1d(np.asarray(own, dtype=np.uint64))
    p = np.atleast_1d(np.asarray(opp, dtype=np.uint64))
    with np.errstate(over="ignore"):
        h = o * np.uint64(0x9E3779B97F4A7C15) ^ (p + np.uint64(0xD1B54A32D192ED03)) * np.uint64(0xBF58476D1CE4E5B9)
        h = h ^ (h >> np.uint64(29))
        h = h * np.uint64(0x94D049BB133111EB)
        h = h ^ (h >> np.uint64(32))
    s = ((h & LOW) & np.uint64(mask)).astype(np.int64)
    return int(s[0]) if scalar else s


def seq_word(seq, writer=0):
    return (int(writer) << 32) | int(seq)


def value_word(seq, bits):
    return (int(seq) << 32) | int(bits)


def float_bits(x):
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def _signed(x):
    x = int(x) & 0xFFFFFFFFFFFFFFFF
    return x - (1 << 64) if x >= 1 << 63 else x


def plant(m, slot, seq_w, own, opp, value_w):
    """Write the four words of entry `slot` of m's table from the host (before a launch)."""
    tab = m._vtable.view(-1, 4)
    assert 0 <= slot < tab.shape[0]
    tab[slot] = torch.tensor([_signed(seq_w), _signed(own), _signed(opp), _signed(value_w)], dtype=torch.int64,
                             device=tab.device)
    torch.cuda.synchronize()


def read(m):
    """Host copy of m's table: uint64 [slots][4]."""
    torch.cuda.synchronize()
    return m._vtable.cpu().numpy().view(np.uint64).reshape(-1, 4).copy()


def writers_of(m):
    """The sequence words' high halves a launch of m can write: the slots of its games (a wave search: games x width)."""
    return m.n_games * (m.wave if getattr(m, "wave_entry", False) else 1)


def audit(table, value, n_writers=None, n_walk=None):
    """Every entry in use (sequence word non-zero) of the table after a launch -- an engine, or a host array uint64
    [slots][4] -- is a published one of a position of the run, holds the value net's value of that position and lies
    where a lookup looks for it:

      * the sequence word is even; the value word's high half is the sequence word's low half;
      * the writer is below n_writers (default: writers_of(the engine));
      * own & opp == 0;
      * the entry's index is slot_of(own, opp, slots - 1);
      * the value bits equal, bit for bit, value.forward_boards_counted of (own, opp): n_walk = None -- every entry,
        all of them in one launch; n_walk = k -- at most k entries drawn without replacement (RandomState(5)), ONE
        board per launch (the one-board walk: what the oracle's value_fn takes).

    Returns (entries in use, entries walked)."""
    from iago_amd import ops
    if hasattr(table, "_vtable"):
        n_writers = writers_of(table) if n_writers is None else n_writers
        tab = read(table)
    else:
        tab = np.asarray(table).view(np.uint64).reshape(-1, 4)
    assert n_writers is not None
    slots = tab.shape[0]
    assert slots > 0 and slots & (slots - 1) == 0
    seq, own, opp, val = tab[:, 0], tab[:, 1], tab[:, 2], tab[:, 3]
    used = np.nonzero(seq)[0]
    if len(used) == 0:
        return 0, 0
    assert not np.any(seq[used] & np.uint64(1)), "an entry was left with an odd sequence word"
    assert np.array_equal(val[used] >> np.uint64(32), seq[used] & LOW), "value word / sequence word mismatch"
    writer = (seq[used] >> np.uint64(32)).astype(np.int64)
    assert writer.min() >= 0 and writer.max() < n_writers        # the game that asked (or walked ahead)
    assert not np.any(own[used] & opp[used])                     # positions: disjoint stones
    home = slot_of(own[used], opp[used], slots - 1)
    lost = np.nonzero(home != used)[0]
    assert len(lost) == 0, "%d of %d entries lie in a slot no lookup of their position reads (first: slot %d, home %d)" % (
        len(lost), len(used), int(used[lost[0]]), int(home[lost[0]]))
    if n_walk is None:
        pick = used
    else:
        rs = np.random.RandomState(5)
        pick = used if len(used) <= n_walk else rs.choice(used, n_walk, replace=False)
    n = len(pick)
    o, p = ops.bits_to_tensor(own[pick]), ops.bits_to_tensor(opp[pick])
    idx = torch.arange(n, dtype=torch.int64, device="cuda")
    out = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    with torch.no_grad():
        if n_walk is None:
            value.forward_boards_counted(o, p, idx, torch.full((1,), n, dtype=torch.int32, device="cuda"), out)
        else:
            one = torch.ones(1, dtype=torch.int32, device="cuda")
            for i in range(n):      # ONE board per launch: the one-board walk (value to out[index[0]])
                value.forward_boards_counted(o, p, idx[i:i + 1], one, out)
    got = out.cpu().numpy().view(np.uint32)
    want = (val[pick] & LOW).astype(np.uint32)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "%d of %d table values differ from the value net's walk of their position (first: slot %d)" % (
        len(bad), n, int(pick[bad[0]]))
    return len(used), n
