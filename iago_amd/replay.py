"""A replay window over the rows of recent self-play rounds, and minibatches out of it in random board symmetries.

The window is a ring of `capacity` rows on one device: own / opp (the searched position, own = the mover), pi (the
root's visit counts by cell), move (the move played) and z (the result from the mover's view) -- the columns of
engine.SelfPlayResult.tuples().  Row r of everything ever added lives in slot r % capacity.  `add` is plain torch
indexing and works on any device; `sample` and `gather` run iago_replay_sample (include/iago_hip_training.h) and
need the GPU: one launch draws the rows, with replacement, and turns each into one of the board's eight symmetries,
position, visit row and move together.  The draw is in integers and keyed by Philox on (row of the minibatch, step)
under the window's seed: it depends on nothing else, so the ranks of a multi-GPU run, whose windows hold the same rows
in the same slots (train_rl.ReinforceTrainer.add_to_window), draw the same minibatch.
"""
import torch

from . import _lib, ops

COLUMNS = (("own", torch.int64), ("opp", torch.int64), ("pi", torch.int32), ("move", torch.int8), ("z", torch.int8))


class ReplayWindow(object):
    """ReplayWindow(capacity, seed=0, device="cuda"): `count` slots are filled (at most capacity), `total` rows were
    ever added, `step` is the counter the next sample(n) without a step of its own is keyed by."""

    def __init__(self, capacity, seed=0, device="cuda"):
        capacity = int(capacity)
        if not 1 <= capacity < 2 ** 31:
            raise ValueError("ReplayWindow: capacity must be in [1, 2^31), got %r" % (capacity,))
        self.capacity, self.seed, self.device = capacity, int(seed), torch.device(device)
        self.total, self.step = 0, 0
        self.cols = {k: torch.zeros((capacity, 64) if k == "pi" else (capacity,), dtype=dt, device=self.device)
                     for k, dt in COLUMNS}
        self._flags = None

    @property
    def count(self):
        return min(self.total, self.capacity)

    def add(self, tup):
        """Append the rows of a SelfPlayResult.tuples() dict (own, opp, pi, move, z; other keys are ignored), in their
        order.  Of a batch larger than the window its last `capacity` rows stay."""
        n = int(tup["own"].numel())
        rows = {}
        for k, dt in COLUMNS:
            t = tup[k]
            if t.shape[0] != n or (k == "pi" and tuple(t.shape) != (n, 64)):
                raise ValueError("ReplayWindow.add: %s has shape %s for %d rows" % (k, tuple(t.shape), n))
            rows[k] = t.to(device=self.device, dtype=dt)
        first = max(n - self.capacity, 0)                        # (rows before it would be overwritten by later ones)
        slots = (torch.arange(self.total + first, self.total + n, device=self.device)) % self.capacity
        for k, _ in COLUMNS:
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
        return out

    def sample(self, n, step=None):
        """n rows drawn with replacement, each in a drawn symmetry: a dict own, opp, pi, move, z, result (float32 z, the
        Value net's label), slot, sym.  step None: the window's own counter, which then advances by one."""
        self._not_empty()
        if step is None:
            step = self.step
            self.step += 1
        return self._run(int(n), step, None, None)

    def gather(self, slot, sym):
        """The rows of the given slots in the given variants: slot (n,) integers or a tensor, sym the same or one int
        for every row."""
        self._not_empty()
        slot = torch.as_tensor(slot, device=self.device).to(torch.int32).reshape(-1).contiguous()
        if isinstance(sym, int):
            sym = torch.full((slot.numel(),), sym, dtype=torch.uint8, device=self.device)
        sym = torch.as_tensor(sym, device=self.device).to(torch.uint8).reshape(-1).contiguous()
        return self._run(slot.numel(), 0, slot, sym)
