"""A replay window over the rows of recent self-play rounds, and minibatches out of it in random board symmetries.

The window is a ring of `capacity` rows on one device: own / opp (the searched position, own = the mover), pi (the
root's visit counts by cell), move (the move played) and z (the result from the mover's view) -- the columns of
engine.SelfPlayResult.tuples().  Row r of everything ever added lives in slot r % capacity.  `add` is plain torch
indexing and works on any device; `sample` and `gather` run iago_replay_sample (include/iago_hip_training.h) and
need the GPU: one launch draws the rows, with replacement, and turns each into one of the board's eight symmetries,
position, visit row and move together.  The draw is in integers and keyed by Philox on (row of the minibatch, step)
under the window's seed: it depends on nothing else, so the ranks of a multi-GPU run, whose windows hold the same rows
in the same slots (train_rl.ReinforceTrainer.add_to_window), draw the same minibatch.

Self-play repeats itself: every game opens on the same position, and after one ply there is one position up to the
board's symmetries.  `merge` groups the rows by canonical position (iago_canonical_rows: the smallest of the eight
variants), sums each group's visit rows in the canonical frame and its results (iago_replay_merge), and
`sample(merged="unique" | "rows")` draws out of those groups (iago_replay_sample_merged): the targets of a position are
then the sum of its searches and its measured mean result, not one noisy copy of either.

ReplayWindow(value_targets=True) holds one more column, v: the rows' value targets (int32, Q16, from the mover's view --
engine.SelfPlayResult.tuples(value_target=(lam_256, mix_256)), iago_value_targets), the Value net's label in place of z.
A value is invariant under the board's symmetries, so the plain draw gathers v by the slot the kernel returns, and a
merged position's label is the mean of its rows' v (iago_replay_merge_values sums them in 64 bits).
"""
import torch

from . import _lib, ops

COLUMNS = (("own", torch.int64), ("opp", torch.int64), ("pi", torch.int32), ("move", torch.int8), ("z", torch.int8))
MERGED_COLUMNS = ("own", "opp", "pi", "z_sum", "mult", "first")
VALUE_COLUMN = ("v", torch.int32)   # ReplayWindow(value_targets=True): the rows' value targets, Q16


class MergedRows(object):
    """A window merged by position up to symmetry (ReplayWindow.merge, iago_replay_merge): n_unique groups, one per
    distinct canonical position, in ascending (own, opp) as unsigned 64-bit.  own / opp: the canonical boards; pi
    (n_unique, 64) int32: the group's visit rows, each turned into the canonical frame, summed; z_sum int32: its
    results summed; mult int32: its rows; first int64: the exclusive prefix sum of mult.  count / total: the window's
    when the snapshot was taken.  v_sum int64: the group's value targets summed (iago_replay_merge_values), of a window
    with value targets; None of any other."""

    def __init__(self, n_unique, count, total, own, opp, pi, z_sum, mult, first, v_sum=None):
        self.n_unique, self.count, self.total = int(n_unique), int(count), int(total)
        self.own, self.opp, self.pi, self.z_sum, self.mult, self.first = own, opp, pi, z_sum, mult, first
        self.v_sum = v_sum


class ReplayWindow(object):
    """ReplayWindow(capacity, seed=0, device="cuda", value_targets=False): `count` slots are filled (at most capacity),
    `total` rows were ever added, `step` is the counter the next sample(n) without a step of its own is keyed by.
    value_targets = True: the window also holds the int32 column v, the rows' value targets in Q16 -- add() then needs
    it, and sample()'s `result` is made of it, not of z."""

    def __init__(self, capacity, seed=0, device="cuda", value_targets=False):
        capacity = int(capacity)
        if not 1 <= capacity < 2 ** 31:
            raise ValueError("ReplayWindow: capacity must be in [1, 2^31), got %r" % (capacity,))
        self.capacity, self.seed, self.device = capacity, int(seed), torch.device(device)
        self.total, self.step = 0, 0
        self.value_targets = bool(value_targets)
        self.columns = COLUMNS + ((VALUE_COLUMN,) if self.value_targets else ())
        self.cols = {k: torch.zeros((capacity, 64) if k == "pi" else (capacity,), dtype=dt, device=self.device)
                     for k, dt in self.columns}
        self._flags = None
        self._merged = None

    @property
    def count(self):
        return min(self.total, self.capacity)

    def add(self, tup):
        """Append the rows of a SelfPlayResult.tuples() dict (own, opp, pi, move, z; other keys are ignored), in their
        order.  Of a batch larger than the window its last `capacity` rows stay.  A window with value targets also takes
        v (tuples(value_target=...)) and refuses a dict without it."""
        if self.value_targets and "v" not in tup:
            raise ValueError("ReplayWindow.add: a window with value targets needs the column v "
                             "(SelfPlayResult.tuples(value_target=(lam_256, mix_256)))")
        n = int(tup["own"].numel())
        rows = {}
        for k, dt in self.columns:
            t = tup[k]
            if t.shape[0] != n or (k == "pi" and tuple(t.shape) != (n, 64)):
                raise ValueError("ReplayWindow.add: %s has shape %s for %d rows" % (k, tuple(t.shape), n))
            rows[k] = t.to(device=self.device, dtype=dt)
        first = max(n - self.capacity, 0)                        # (rows before it would be overwritten by later ones)
        slots = (torch.arange(self.total + first, self.total + n, device=self.device)) % self.capacity
        for k, _ in self.columns:
            self.cols[k][slots] = rows[k][first:]
        self.total += n
        return n

    def _not_empty(self):
        if self.total == 0:
            raise ValueError("ReplayWindow: the window is empty")

    def _run(self, n, step, slot, sym):
        if self._flags is None:
            self._flags = torch.zeros(1, dtype=torch.int32, device=self.device)
        c = self.cols
        out = ops.replay_sample(c["own"], c["opp"], c["pi"], c["move"], c["z"], self.count, n=n, seed=self.seed,
                                step=step, slot=slot, sym=sym, flags=self._flags)
        if int(self._flags.item()):
            self._flags.zero_()
            raise _lib.IagoError("ReplayWindow: a slot lies outside the %d filled slots or a variant outside 0 .. 7; "
                                 "those rows came back as zeros" % self.count)
        if self.value_targets:   # (a value does not turn with the board: gathered by the slot the kernel returns)
            out["v"] = c["v"][out["slot"].to(torch.int64)]
            out["result"] = out["v"].to(torch.float32) / _lib.VALUE_Q16   # (exact for |v| <= 2^24)
        return out

    def merge(self):
        """The filled slots merged by position up to symmetry (iago_replay_merge): a MergedRows snapshot of the window
        as it stands, one row per distinct canonical position.  One readback, of n_unique and the flags.  A summed
        cell beyond int32 raises IagoError."""
        self._not_empty()
        c = self.cols
        m = ops.replay_merge(c["own"], c["opp"], c["pi"], c["z"], self.count)
        n_unique, flags = m["meta"].tolist()
        if flags & _lib.REPLAY_MERGE_OVERFLOW:
            raise _lib.IagoError("ReplayWindow.merge: a summed visit count or result left int32 (2^31 - 1)")
        if flags or not 1 <= n_unique <= self.count:
            raise _lib.IagoError("ReplayWindow.merge: the device refused the rows' order (flags %d, %d groups)"
                                 % (flags, n_unique))
        v_sum = None
        if self.value_targets:
            v_sum = ops.replay_merge_values(m["order"], m["group"], m["first"][:n_unique], m["mult"][:n_unique], c["v"])
        return MergedRows(n_unique=n_unique, count=self.count, total=self.total, v_sum=v_sum,
                          **{k: m[k][:n_unique] for k in MERGED_COLUMNS})

    def merged(self):
        """merge(), kept until rows are added: the snapshot the merged draws read."""
        if self._merged is None or self._merged.total != self.total:
            self._merged = None   # (the old snapshot's buffers go before the new one's are made)
            self._merged = self.merge()
        return self._merged

    def sample(self, n, step=None, merged=None):
        """n rows drawn with replacement, each in a drawn symmetry: a dict own, opp, pi, move, z, result (float32 z, the
        Value net's label), slot, sym.  step None: the window's own counter, which then advances by one.
        On a window with value targets the dict also has v (int32, Q16: the row's value target, gathered by slot) and
        result = float32(v) / 65536, which is exact for |v| <= 2^24 (a target never exceeds 2^16).

        merged = "unique" or "rows" draws out of the window merged by position up to symmetry (merged(): rebuilt on
        the first such draw after rows were added) with iago_replay_sample_merged, under the same key and counter:
        "unique" uniformly over the distinct positions, "rows" uniformly over the window's rows, each standing for
        its position.  The dict is then own, opp, pi (the position's summed visit rows, int32), result (float32, the
        mean of its rows' z), z_sum, mult, group, sym: a merged row has no move and no z.  On a window with value
        targets also v_sum (int64: the position's value targets summed) and result = float32(float64(v_sum) / (65536 *
        mult)), the mean target -- one float64 division (exact operands), one rounding to float32."""
        if merged not in (None, "unique", "rows"):
            raise ValueError("ReplayWindow.sample: merged must be None, 'unique' or 'rows', got %r" % (merged,))
        self._not_empty()
        m = self.merged() if merged is not None else None
        if step is None:
            step = self.step
            self.step += 1
        if m is None:
            return self._run(int(n), step, None, None)
        out = ops.replay_sample_merged(m.own, m.opp, m.pi, m.z_sum, m.mult, m.first, m.count, n, seed=self.seed,
                                       step=step, mode=merged)
        if self.value_targets:
            out["v_sum"] = m.v_sum[out["group"].to(torch.int64)]
            out["result"] = (out["v_sum"].to(torch.float64)
                             / (float(_lib.VALUE_Q16) * out["mult"].to(torch.float64))).to(torch.float32)
        return out

    def gather(self, slot, sym):
        """The rows of the given slots in the given variants: slot (n,) integers or a tensor, sym the same or one int
        for every row."""
        self._not_empty()
        slot = torch.as_tensor(slot, device=self.device).to(torch.int32).reshape(-1).contiguous()
        if isinstance(sym, int):
            sym = torch.full((slot.numel(),), sym, dtype=torch.uint8, device=self.device)
        sym = torch.as_tensor(sym, device=self.device).to(torch.uint8).reshape(-1).contiguous()
        return self._run(slot.numel(), 0, slot, sym)
