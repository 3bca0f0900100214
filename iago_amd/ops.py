"""Tensor-level wrappers over the C ABI (include/iago_hip.h).

Boards are int64 CUDA tensors holding the 64-bit bitboards (bit a = row*8+col;
`own` = side to move).  Every function launches on torch's current stream and
requires CUDA tensors: there is no CPU path.
"""
import ctypes as C
import numbers

import numpy as np
import torch

from . import _lib
from ._lib import IAGO_MAX_TURNS, IAGO_ROLLOUT_TABLE_FLOATS, RolloutArgs, check


try:   # (torch.cuda.current_stream() costs ~8 us of Python per call: 40 % of a small launch's host time)
    _raw_stream, _cur_device = torch._C._cuda_getCurrentRawStream, torch._C._cuda_getDevice
except AttributeError:  # a torch without these internals
    _raw_stream = _cur_device = None


def _stream():
    """The current HIP stream of the current device as a void* for the C ABI."""
    if _raw_stream is not None:
        return C.c_void_p(_raw_stream(_cur_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t, dtype, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.IagoError("%s must be a CUDA tensor (the HIP path has no CPU fallback)" % name)
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    return C.c_void_p(t.data_ptr())


def bits_to_tensor(values, device="cuda"):
    """Python ints / numpy uint64 -> int64 tensor with the same bit patterns."""
    a = np.asarray(values, dtype=np.uint64).reshape(-1)
    return torch.from_numpy(a.view(np.int64).copy()).to(device)


def tensor_to_bits(t):
    """int64 tensor -> numpy uint64 array."""
    return t.detach().cpu().numpy().view(np.uint64)


def legal_moves(own, opp):
    """Bit mask of legal moves per board (game.py:210-235, rl_env.py:114-138)."""
    n = own.numel()
    out = torch.empty_like(own)
    check(_lib.lib().iago_legal_moves(_dev(own, torch.int64, "own"), _dev(opp, torch.int64, "opp"),
                                      _dev(out, torch.int64, "legal"), n, _stream()),
          "iago_legal_moves")
    return out


def apply_moves(own, opp, action):
    """In place place_stone (game.py:180-207); action int8, -1 = pass."""
    n = own.numel()
    if action.numel() != n or opp.numel() != n:
        raise ValueError("own/opp/action sizes differ")
    check(_lib.lib().iago_apply_moves(_dev(own, torch.int64, "own"), _dev(opp, torch.int64, "opp"),
                                      _dev(action, torch.int8, "action"), n, _stream()),
          "iago_apply_moves")
    return own, opp


def play_turn(own, opp, action, active, stone_num, pass_flg, done, close_pair, legal, active_next):
    """One turn of n lockstep games in place (iago_play_turn): the move, stone_num / pass_flg /
    done, the swap of sides (own = the next mover afterwards), the next mover's legal moves and
    the next turn's `active`.  uint8 flags, int32 stone_num, int8 action."""
    n = own.numel()
    for name, t in (("opp", opp), ("action", action), ("active", active), ("stone_num", stone_num),
                    ("pass_flg", pass_flg), ("done", done), ("legal", legal), ("active_next", active_next)):
        if t.numel() != n:
            raise ValueError("play_turn: %s has %d entries, expected %d" % (name, t.numel(), n))
    if active.data_ptr() == active_next.data_ptr():
        raise ValueError("play_turn: active and active_next may not alias")
    check(_lib.lib().iago_play_turn(_dev(own, torch.int64, "own"), _dev(opp, torch.int64, "opp"),
                                    _dev(action, torch.int8, "action"), _dev(active, torch.uint8, "active"),
                                    _dev(stone_num, torch.int32, "stone_num"), _dev(pass_flg, torch.uint8, "pass_flg"),
                                    _dev(done, torch.uint8, "done"), 1 if close_pair else 0,
                                    _dev(legal, torch.int64, "legal"), _dev(active_next, torch.uint8, "active_next"),
                                    n, _stream()), "iago_play_turn")


def encode_planes(own, opp, out=None):
    """(n,2,8,8) float32 planes, channel 0 = opp, channel 1 = own (game.py:168-174)."""
    n = own.numel()
    if out is None:
        out = torch.empty((n, 2, 8, 8), dtype=torch.float32, device=own.device)
    elif out.numel() != n * 128:
        raise ValueError("planes buffer has the wrong size")
    check(_lib.lib().iago_encode_planes(_dev(own, torch.int64, "own"),
                                        _dev(opp, torch.int64, "opp"),
                                        _dev(out, torch.float32, "planes"), n, _stream()),
          "iago_encode_planes")
    return out


def _count(n_dev):
    """Optional int32 CUDA word holding a device-side item count (iago_hip.h, `n_dev`)."""
    return _dev(n_dev, torch.int32, "n_dev") if n_dev is not None else None


def encode_planes_indexed(own, opp, index, out, n_dev=None):
    """Planes of boards index[0..k) (int64 tensor) into out[:k] (game.py:168-174); with
    n_dev only the first min(k, *n_dev) rows."""
    k = index.numel()
    if out.numel() < k * 128:
        raise ValueError("planes buffer is too small")
    check(_lib.lib().iago_encode_planes_indexed(_dev(own, torch.int64, "own"), _dev(opp, torch.int64, "opp"),
                                                _dev(index, torch.int64, "index"),
                                                _dev(out, torch.float32, "planes"), k, _count(n_dev),
                                                _stream()),
          "iago_encode_planes_indexed")
    return out


def judge(own, opp):
    """sign(#own - #opp) as int8 (mcts_self_play.py:113-121)."""
    n = own.numel()
    out = torch.empty(n, dtype=torch.int8, device=own.device)
    check(_lib.lib().iago_judge(_dev(own, torch.int64, "own"), _dev(opp, torch.int64, "opp"),
                                _dev(out, torch.int8, "z"), n, _stream()), "iago_judge")
    return out


def augment8(own, opp, action):
    """8-fold dihedral augmentation in the reference's order (load.py:56-74):
    returns (8, n) own, opp (int64) and action (int8)."""
    n = own.numel()
    oo = torch.empty((8, n), dtype=torch.int64, device=own.device)
    po = torch.empty((8, n), dtype=torch.int64, device=own.device)
    ao = torch.empty((8, n), dtype=torch.int8, device=own.device)
    check(_lib.lib().iago_augment8(_dev(own, torch.int64, "own"), _dev(opp, torch.int64, "opp"),
                                   _dev(action, torch.int8, "action"), _dev(oo, torch.int64, "o"),
                                   _dev(po, torch.int64, "p"), _dev(ao, torch.int8, "a"), n,
                                   _stream()), "iago_augment8")
    return oo, po, ao


def replay_sample(own, opp, pi, move, z, count, n=None, seed=0, step=0, slot=None, sym=None, flags=None):
    """iago_replay_sample (include/iago_hip_training.h): n rows out of the window own / opp (capacity,) int64, pi
    (capacity, 64) int32, move / z (capacity,) int8 whose slots 0 .. count-1 are filled, every row in one of the
    board's eight symmetries (ops.augment8's variants) -- position, visit row and move together.  slot / sym None: row
    j's slot and variant are drawn from Philox on (j, step) under seed ^ (REPLAY_KEY << 32), with replacement; slot
    (n,) int32 and sym (n,) uint8: those are taken (n defaults to their length).  flags: optional int32 word, or-ed
    into -- bit 0: a supplied slot or variant was out of range (that row is zeros, move -1).  Returns a dict own,
    opp, pi, move, z, result (float32 z), slot, sym."""
    capacity = own.numel()
    for name, t in (("opp", opp), ("move", move), ("z", z)):
        if t.numel() != capacity:
            raise ValueError("replay_sample: %s has %d entries, own has %d" % (name, t.numel(), capacity))
    if pi.dim() != 2 or tuple(pi.shape) != (capacity, 64):
        raise ValueError("replay_sample: pi must be (%d, 64), got %s" % (capacity, tuple(pi.shape)))
    if (slot is None) != (sym is None):
        raise ValueError("replay_sample: slot and sym go together (both or neither)")
    if slot is not None:
        if n is None:
            n = slot.numel()
        if slot.numel() != n or sym.numel() != n:
            raise ValueError("replay_sample: slot / sym have %d / %d entries for n = %d" % (slot.numel(), sym.numel(), n))
    if n is None:
        raise ValueError("replay_sample: n is needed where the kernel draws")
    n = int(n)
    dev = own.device
    out = dict(own=torch.empty(n, dtype=torch.int64, device=dev), opp=torch.empty(n, dtype=torch.int64, device=dev),
               pi=torch.empty((n, 64), dtype=torch.int32, device=dev), move=torch.empty(n, dtype=torch.int8, device=dev),
               z=torch.empty(n, dtype=torch.int8, device=dev), result=torch.empty(n, dtype=torch.float32, device=dev),
               slot=torch.empty(n, dtype=torch.int32, device=dev), sym=torch.empty(n, dtype=torch.uint8, device=dev))
    a = _lib.ReplaySampleArgs()
    a.own, a.opp, a.pi = _dev(own, torch.int64, "own"), _dev(opp, torch.int64, "opp"), _dev(pi, torch.int32, "pi")
    a.move, a.z = _dev(move, torch.int8, "move"), _dev(z, torch.int8, "z")
    a.capacity, a.count, a.n = capacity, int(count), n
    a.seed, a.step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFF
    if slot is not None:
        a.slot_in, a.sym_in = _dev(slot, torch.int32, "slot"), _dev(sym, torch.uint8, "sym")
    a.own_out, a.opp_out, a.pi_out = out["own"].data_ptr(), out["opp"].data_ptr(), out["pi"].data_ptr()
    a.move_out, a.z_out, a.result_out = out["move"].data_ptr(), out["z"].data_ptr(), out["result"].data_ptr()
    a.slot_out, a.sym_out = out["slot"].data_ptr(), out["sym"].data_ptr()
    a.flags = _dev(flags, torch.int32, "flags") if flags is not None else None
    check(_lib.lib().iago_replay_sample(C.byref(a), _stream()), "iago_replay_sample")
    return out


def canonical_rows(own, opp):
    """iago_canonical_rows (include/iago_hip_training.h): per row the smallest of the eight pairs (variant k of own,
    variant k of opp) -- own compared first, then opp, as unsigned 64-bit -- and the lowest k that gives it.  Returns
    (c_own, c_opp) int64 and sym uint8; every symmetry of a position has the same (c_own, c_opp)."""
    n = own.numel()
    if opp.numel() != n:
        raise ValueError("canonical_rows: opp has %d entries, own has %d" % (opp.numel(), n))
    c_own, c_opp = torch.empty_like(own), torch.empty_like(opp)
    sym = torch.empty(n, dtype=torch.uint8, device=own.device)
    check(_lib.lib().iago_canonical_rows(_dev(own, torch.int64, "own"), _dev(opp, torch.int64, "opp"), n,
                                         c_own.data_ptr(), c_opp.data_ptr(), sym.data_ptr(), _stream()),
          "iago_canonical_rows")
    return c_own, c_opp, sym


def _unsigned_order(x):
    """int64 bit patterns as keys whose signed order is the patterns' unsigned order."""
    return x ^ torch.iinfo(torch.int64).min


def replay_merge(own, opp, pi, z, count, meta=None):
    """iago_replay_merge (include/iago_hip_training.h) over the filled slots 0 .. count-1 of the window own / opp
    (capacity,) int64, pi (capacity, 64) int32, z (capacity,) int8: the rows canonicalised (canonical_rows), ordered
    by (c_own, c_opp) as unsigned -- two stable sorts, torch's -- and summed per distinct position on the device.
    meta: optional int32 (2,) tensor, cleared here: [0] receives n_unique, [1] the flags (_lib.REPLAY_MERGE_*).
    Returns a dict own, opp (count,), pi (count, 64) int32, z_sum, mult int32, first int64 -- count-sized buffers
    whose first n_unique entries are the groups, in ascending (own, opp) -- meta, and the order / group (count,) int32
    the merge took (the slots in ascending canonical position and their group numbers: what replay_merge_values sums
    another column by).  Nothing is read back."""
    capacity, count = own.numel(), int(count)
    for name, t in (("opp", opp), ("z", z)):
        if t.numel() != capacity:
            raise ValueError("replay_merge: %s has %d entries, own has %d" % (name, t.numel(), capacity))
    if pi.dim() != 2 or tuple(pi.shape) != (capacity, 64):
        raise ValueError("replay_merge: pi must be (%d, 64), got %s" % (capacity, tuple(pi.shape)))
    if not 1 <= count <= capacity:
        raise ValueError("replay_merge: need 1 <= count <= %d, got %d" % (capacity, count))
    dev = own.device
    c_own, c_opp, sym = canonical_rows(own[:count], opp[:count])
    by_opp = torch.sort(_unsigned_order(c_opp), stable=True)[1]
    order = by_opp[torch.sort(_unsigned_order(c_own)[by_opp], stable=True)[1]]
    so, sp = c_own[order], c_opp[order]
    head = torch.ones(count, dtype=torch.int32, device=dev)
    head[1:] = ((so[1:] != so[:-1]) | (sp[1:] != sp[:-1])).to(torch.int32)
    group = (torch.cumsum(head, 0) - 1).to(torch.int32)
    order = order.to(torch.int32)
    if meta is None:
        meta = torch.empty(2, dtype=torch.int32, device=dev)
    meta.zero_()
    out = dict(own=torch.empty(count, dtype=torch.int64, device=dev), opp=torch.empty(count, dtype=torch.int64, device=dev),
               pi=torch.empty((count, 64), dtype=torch.int32, device=dev),
               z_sum=torch.empty(count, dtype=torch.int32, device=dev), mult=torch.empty(count, dtype=torch.int32, device=dev),
               first=torch.empty(count, dtype=torch.int64, device=dev), meta=meta, order=order, group=group)
    a = _lib.ReplayMergeArgs()
    a.c_own, a.c_opp, a.sym = c_own.data_ptr(), c_opp.data_ptr(), sym.data_ptr()
    a.pi, a.z, a.count = _dev(pi, torch.int32, "pi"), _dev(z, torch.int8, "z"), count
    a.order, a.group = _dev(order, torch.int32, "order"), _dev(group, torch.int32, "group")
    a.own_out, a.opp_out, a.pi_out = out["own"].data_ptr(), out["opp"].data_ptr(), out["pi"].data_ptr()
    a.z_sum, a.mult, a.first = out["z_sum"].data_ptr(), out["mult"].data_ptr(), out["first"].data_ptr()
    _dev(meta, torch.int32, "meta")
    a.n_unique, a.flags = meta.data_ptr(), meta.data_ptr() + 4
    workspace = torch.empty(count, dtype=torch.int64, device=dev)   # (the large groups' 64-bit sums: cleared by the call)
    a.workspace = workspace.data_ptr()
    check(_lib.lib().iago_replay_merge(C.byref(a), _stream()), "iago_replay_merge")
    return out


def replay_sample_merged(own, opp, pi, z_sum, mult, first, count, n, seed=0, step=0, mode="unique"):
    """iago_replay_sample_merged (include/iago_hip_training.h): n rows out of the n_unique = own.numel() merged rows
    of a window of count rows, every row in one of the board's eight symmetries.  Row j's group and variant are drawn
    from replay_sample's Philox stream on (j, step): mode "unique" uniformly over the groups, "rows" uniformly over
    the window's rows (the group that holds the row, by first).  Returns a dict own, opp, pi (int32 sums), result
    (float32 z_sum / mult), z_sum, mult, group, sym."""
    if mode not in _lib.REPLAY_MERGED_MODES:
        raise ValueError("replay_sample_merged: mode must be 'unique' or 'rows', got %r" % (mode,))
    groups, n = own.numel(), int(n)
    for name, t in (("opp", opp), ("z_sum", z_sum), ("mult", mult), ("first", first)):
        if t.numel() != groups:
            raise ValueError("replay_sample_merged: %s has %d entries, own has %d" % (name, t.numel(), groups))
    if pi.dim() != 2 or tuple(pi.shape) != (groups, 64):
        raise ValueError("replay_sample_merged: pi must be (%d, 64), got %s" % (groups, tuple(pi.shape)))
    dev = own.device
    i32 = dict(dtype=torch.int32, device=dev)
    out = dict(own=torch.empty(n, dtype=torch.int64, device=dev), opp=torch.empty(n, dtype=torch.int64, device=dev),
               pi=torch.empty((n, 64), **i32), result=torch.empty(n, dtype=torch.float32, device=dev),
               z_sum=torch.empty(n, **i32), mult=torch.empty(n, **i32), group=torch.empty(n, **i32),
               sym=torch.empty(n, dtype=torch.uint8, device=dev))
    a = _lib.ReplaySampleMergedArgs()
    a.own, a.opp, a.pi = _dev(own, torch.int64, "own"), _dev(opp, torch.int64, "opp"), _dev(pi, torch.int32, "pi")
    a.z_sum, a.mult = _dev(z_sum, torch.int32, "z_sum"), _dev(mult, torch.int32, "mult")
    a.first = _dev(first, torch.int64, "first")
    a.n_unique, a.count, a.n = groups, int(count), n
    a.seed, a.step, a.mode = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFF, _lib.REPLAY_MERGED_MODES[mode]
    a.own_out, a.opp_out, a.pi_out = out["own"].data_ptr(), out["opp"].data_ptr(), out["pi"].data_ptr()
    a.result_out, a.z_sum_out, a.mult_out = out["result"].data_ptr(), out["z_sum"].data_ptr(), out["mult"].data_ptr()
    a.group_out, a.sym_out = out["group"].data_ptr(), out["sym"].data_ptr()
    check(_lib.lib().iago_replay_sample_merged(C.byref(a), _stream()), "iago_replay_sample_merged")
    return out


def replay_merge_values(order, group, first, mult, v, flags=None):
    """iago_replay_merge_values (include/iago_hip_training.h): the int32 column v (by slot; at least count entries) summed
    per group of a merge -- order / group (count,) int32 and first int64 / mult int32 (n_unique,) as replay_merge
    returns them (first / mult cut to the groups).  Returns v_sum (n_unique,) int64: 64-bit integer sums, the same bits
    whatever the schedule.  flags: optional int32 word, or-ed into -- bit 0 (_lib.REPLAY_MERGE_BAD_INPUT): a span, slot or
    group number the device refused."""
    count, groups = order.numel(), first.numel()
    if group.numel() != count or mult.numel() != groups:
        raise ValueError("replay_merge_values: order / group have %d / %d entries, first / mult %d / %d"
                         % (count, group.numel(), groups, mult.numel()))
    if v.dim() != 1 or v.numel() < count:
        raise ValueError("replay_merge_values: v must be a column of at least %d entries, got %s" % (count, tuple(v.shape)))
    v_sum = torch.empty(groups, dtype=torch.int64, device=order.device)
    a = _lib.ReplayMergeValuesArgs()
    a.order, a.group = _dev(order, torch.int32, "order"), _dev(group, torch.int32, "group")
    a.first, a.mult, a.v = _dev(first, torch.int64, "first"), _dev(mult, torch.int32, "mult"), _dev(v, torch.int32, "v")
    a.count, a.n_unique, a.v_sum = count, groups, v_sum.data_ptr()
    a.flags = _dev(flags, torch.int32, "flags") if flags is not None else None
    check(_lib.lib().iago_replay_merge_values(C.byref(a), _stream()), "iago_replay_merge_values")
    return v_sum


def value_rate_arg(x, name):
    """lam_256 / mix_256 of the value targets: an int in [0, 256] (256ths), or ValueError."""
    if isinstance(x, bool) or not isinstance(x, numbers.Integral) or not 0 <= x <= 256:
        raise ValueError("%s must be an int in [0, 256] (256ths), not %r" % (name, x))
    return int(x)


def value_targets(valid, q, score, z, mover, lam_256=256, mix_256=0):
    """iago_value_targets (include/iago_hip_training.h): the Value net's targets of recorded games, (T, B) int32 in Q16
    from the MOVER's view, 0 where there is no row.  valid (T, B) uint8, q (T, B) int32 (the roots' values from the
    mover's view, Q16: SelfPlayResult.q), score (T, B) int8 (None: no solved rows' scores, zeros), z (B,) int8 (colour
    1's view), mover (T,) int8 tensor or a sequence of colours 1 / 2.  lam_256 / mix_256 in [0, 256]: TD(lambda)'s lambda
    and the weight of the row's own value, in 256ths -- (256, 0) is 65536 z from the mover's view."""
    lam_256, mix_256 = value_rate_arg(lam_256, "lam_256"), value_rate_arg(mix_256, "mix_256")
    if valid.dim() != 2:
        raise ValueError("value_targets: valid must be (T, B), got %s" % (tuple(valid.shape),))
    T, B = valid.shape
    dev = valid.device
    if score is None:
        score = torch.zeros((T, B), dtype=torch.int8, device=dev)
    if not isinstance(mover, torch.Tensor):
        mover = torch.tensor(list(mover), dtype=torch.int8, device=dev)
    for name, t, shape in (("q", q, (T, B)), ("score", score, (T, B)), ("z", z, (B,)), ("mover", mover, (T,))):
        if tuple(t.shape) != shape:
            raise ValueError("value_targets: %s must be %s, got %s" % (name, shape, tuple(t.shape)))
    out = torch.empty((T, B), dtype=torch.int32, device=dev)
    a = _lib.ValueTargetsArgs()
    a.valid, a.q, a.score = _dev(valid, torch.uint8, "valid"), _dev(q, torch.int32, "q"), _dev(score, torch.int8, "score")
    a.z, a.mover = _dev(z, torch.int8, "z"), _dev(mover, torch.int8, "mover")
    a.n_turns, a.n_games, a.lam_256, a.mix_256, a.out = T, B, lam_256, mix_256, out.data_ptr()
    check(_lib.lib().iago_value_targets(C.byref(a), _stream()), "iago_value_targets")
    return out


def mcts_root_value(tree, active, q16=None, n=None, flags=None):
    """iago_mcts_root_value (include/iago_hip_serving.h): after a search under the negamax backup, per game with
    active[g] != 0 the root's value for the root's mover in Q16 -- rint(-root.q * 65536), saturated to +-2^30 -- and the
    root's visits; 0 and 0 for the others.  tree: a pointer to the iago_mcts_tree (TreePool.ref()); active (n_games,)
    uint8.  q16 / n: (n_games,) int32 buffers to fill (None: fresh ones).  flags: optional int32 word, or-ed into (_lib.ROOT_VALUE_SATURATED, _NAN).
    Returns (q16, n)."""
    games, dev = active.numel(), active.device
    if games != tree._obj.n_games:   # (the kernel walks the tree's games)
        raise ValueError("mcts_root_value: active has %d entries for %d games" % (games, tree._obj.n_games))
    q16 = torch.empty(games, dtype=torch.int32, device=dev) if q16 is None else q16
    n = torch.empty(games, dtype=torch.int32, device=dev) if n is None else n
    if q16.numel() != games or n.numel() != games:
        raise ValueError("mcts_root_value: q16 / n have %d / %d entries for %d games" % (q16.numel(), n.numel(), games))
    check(_lib.lib().iago_mcts_root_value(tree, _dev(active, torch.uint8, "active"), _dev(q16, torch.int32, "q16"),
                                          _dev(n, torch.int32, "n"),
                                          _dev(flags, torch.int32, "flags") if flags is not None else None, _stream()),
          "iago_mcts_root_value")
    return q16, n


def augment8_visits(own, opp, action, pi):
    """ops.augment8 with the rows' visit counts: (8, n) own, opp (int64) and action (int8) in augment8's layout, and
    (8, n, 64) int32 visit rows -- pi[v, i, m_v(a)] = pi[i, a].  iago_replay_sample's given mode over the n rows as a
    window: slot = i, sym = v."""
    n = own.numel()
    dev = own.device
    slot = torch.arange(n, dtype=torch.int32, device=dev).repeat(8)
    sym = torch.arange(8, dtype=torch.uint8, device=dev).repeat_interleave(n)
    z = torch.zeros(n, dtype=torch.int8, device=dev)
    r = replay_sample(own, opp, pi, action, z, n, slot=slot, sym=sym)
    return r["own"].reshape(8, n), r["opp"].reshape(8, n), r["move"].reshape(8, n), r["pi"].reshape(8, n, 64)


def bias_relu_(x, bias):
    """In place max(x + bias[c], 0) on a (n, C, 8, 8) float32 tensor: the epilogue
    of network.Block (network.py:9-13) as one pass."""
    if x.dim() != 4 or x.shape[2] != 8 or x.shape[3] != 8:
        raise ValueError("x must be (n, C, 8, 8)")
    check(_lib.lib().iago_bias_relu(_dev(x, torch.float32, "x"), _dev(bias, torch.float32, "bias"),
                                    x.shape[0], x.shape[1], _stream()), "iago_bias_relu")
    return x


# ---- split-f16 convolution stack (csrc/conv_kernels.hip) --------------------------

class SplitActs(object):
    """Activations in split channel blocks: f16 tensors hi, lo of shape
    (n, C/16, 64, 16); value = hi + lo * 2**-11 (include/iago_hip.h)."""

    __slots__ = ("hi", "lo", "channels")

    def __init__(self, hi, lo, channels):
        self.hi, self.lo, self.channels = hi, lo, channels

    @property
    def n(self):
        return self.hi.shape[0]


def split_weights(weight):
    """(cout, cin, 3, 3) float32 conv weight -> (w_hi, w_lo) f16 tensors
    [cin/16][3][3][cout][16] as iago_conv3x3_split expects them."""
    cout, cin, kh, kw = weight.shape
    if (kh, kw) != (3, 3) or cin % 16 or cout != 128:
        raise ValueError("split_weights: need a (128, 16k, 3, 3) weight")
    w = weight.detach().to(torch.float32).permute(2, 3, 0, 1)          # ky, kx, co, ci
    w = w.reshape(3, 3, cout, cin // 16, 16).permute(3, 0, 1, 2, 4).contiguous()
    hi = w.to(torch.float16)
    lo = ((w - hi.to(torch.float32)) * 2048.0).to(torch.float16)
    return hi.contiguous(), lo.contiguous()


def _flag(overflow):
    """Optional int32 CUDA word the split-f16 kernels raise on saturation (iago_hip.h)."""
    return _dev(overflow, torch.int32, "overflow") if overflow is not None else None


def split_nchw(x, overflow=None):
    """(n, C, 8, 8) float32 -> SplitActs."""
    n, c = x.shape[0], x.shape[1]
    if x.dim() != 4 or x.shape[2] != 8 or x.shape[3] != 8 or c % 16:
        raise ValueError("x must be (n, 16k, 8, 8)")
    hi = torch.empty((n, c // 16, 64, 16), dtype=torch.float16, device=x.device)
    lo = torch.empty_like(hi)
    check(_lib.lib().iago_split_nchw(_dev(x, torch.float32, "x"), _dev(hi, torch.float16, "hi"),
                                     _dev(lo, torch.float16, "lo"), n, c, _flag(overflow), _stream()),
          "iago_split_nchw")
    return SplitActs(hi, lo, c)


def merge_nchw(a):
    """SplitActs -> (n, C, 8, 8) float32."""
    y = torch.empty((a.n, a.channels, 8, 8), dtype=torch.float32, device=a.hi.device)
    check(_lib.lib().iago_merge_nchw(_dev(a.hi, torch.float16, "hi"), _dev(a.lo, torch.float16, "lo"),
                                     _dev(y, torch.float32, "y"), a.n, a.channels, _stream()),
          "iago_merge_nchw")
    return y


def conv3x3_split_trunk(a, layers, overflow=None):
    """Consecutive conv3x3_split layers in one launch.  layers: list of (w_hi, w_lo, bias);
    the first reads SplitActs `a`, each next one its predecessor's output."""
    n = a.n
    descs = (_lib.ConvSplitLayer * len(layers))()
    keep = []
    cur, cin = a, a.channels
    for k, (w_hi, w_lo, bias) in enumerate(layers):
        if w_hi.shape != (cin // 16, 3, 3, 128, 16):
            raise ValueError("layer %d: weight blocks %s do not match %d input channels"
                             % (k, tuple(w_hi.shape), cin))
        hi = torch.empty((n, 8, 64, 16), dtype=torch.float16, device=a.hi.device)
        lo = torch.empty_like(hi)
        d = descs[k]
        d.x_hi, d.x_lo = cur.hi.data_ptr(), cur.lo.data_ptr()
        d.w_hi, d.w_lo = _dev(w_hi, torch.float16, "w_hi").value, _dev(w_lo, torch.float16, "w_lo").value
        d.bias = _dev(bias, torch.float32, "bias").value
        d.y_hi, d.y_lo = hi.data_ptr(), lo.data_ptr()
        d.cin = cin
        cur, cin = SplitActs(hi, lo, 128), 128
        keep.append(cur)
    check(_lib.lib().iago_conv3x3_split_trunk(descs, len(layers), n, _flag(overflow), _stream()),
          "iago_conv3x3_split_trunk")
    return cur


def value_stem(planes, w1, b1, overflow=None):
    """relu(conv3x3(planes, w1) + b1), 2 -> 64 channels (Value.block1, network.py:68-70):
    float32 planes (n, 2, 8, 8) -> SplitActs with 64 channels."""
    n = planes.shape[0]
    if tuple(planes.shape[1:]) != (2, 8, 8) or tuple(w1.shape) != (64, 2, 3, 3):
        raise ValueError("value_stem: planes (n,2,8,8) and w1 (64,2,3,3) expected")
    hi = torch.empty((n, 4, 64, 16), dtype=torch.float16, device=planes.device)
    lo = torch.empty_like(hi)
    check(_lib.lib().iago_value_stem(_dev(planes, torch.float32, "planes"), _dev(w1, torch.float32, "w1"),
                                     _dev(b1, torch.float32, "b1"), _dev(hi, torch.float16, "y_hi"),
                                     _dev(lo, torch.float16, "y_lo"), n, _flag(overflow), _stream()),
          "iago_value_stem")
    return SplitActs(hi, lo, 64)


def value_stem_boards(own, opp, w1, b1, overflow=None):
    """value_stem on the boards themselves (own = side to move): plane encoding fused in."""
    n = own.numel()
    hi = torch.empty((n, 4, 64, 16), dtype=torch.float16, device=own.device)
    lo = torch.empty_like(hi)
    check(_lib.lib().iago_value_stem_boards(_dev(own, torch.int64, "own"), _dev(opp, torch.int64, "opp"),
                                            _dev(w1, torch.float32, "w1"), _dev(b1, torch.float32, "b1"),
                                            _dev(hi, torch.float16, "y_hi"), _dev(lo, torch.float16, "y_lo"),
                                            n, _flag(overflow), _stream()), "iago_value_stem_boards")
    return SplitActs(hi, lo, 64)


def value_head(a, w9, b9, w10, w11):
    """Value.block9 + fc10 + fc11 with train=False (network.py:78-96) on SplitActs with
    128 channels -> (n,) float32."""
    if a.channels != 128 or tuple(w9.shape) != (1, 128, 3, 3) or tuple(w10.shape) != (128, 64) \
            or tuple(w11.shape) != (1, 128):
        raise ValueError("value_head: unexpected shapes")
    out = torch.empty((a.n,), dtype=torch.float32, device=a.hi.device)
    check(_lib.lib().iago_value_head(_dev(a.hi, torch.float16, "x_hi"), _dev(a.lo, torch.float16, "x_lo"),
                                     _dev(w9, torch.float32, "w9"), _dev(b9, torch.float32, "b9"),
                                     _dev(w10, torch.float32, "w10"), _dev(w11, torch.float32, "w11"),
                                     _dev(out, torch.float32, "out"), a.n, _stream()), "iago_value_head")
    return out


def split_weights3(weight):
    """(128, cin, 3, 3) float32 conv weight -> (w_hi, w_mid, w_lo) f16 tensors
    [cin/16][3][3][128][16] with w == hi + mid 2^-11 + lo 2^-22 exactly
    (iago_policy_forward_split3)."""
    cout, cin, kh, kw = weight.shape
    if (kh, kw) != (3, 3) or cin % 16 or cout != 128:
        raise ValueError("split_weights3: need a (128, 16k, 3, 3) weight")
    w = weight.detach().to(torch.float32).permute(2, 3, 0, 1)          # ky, kx, co, ci
    w = w.reshape(3, 3, cout, cin // 16, 16).permute(3, 0, 1, 2, 4).contiguous()
    hi = w.to(torch.float16)
    r1 = (w - hi.to(torch.float32)) * 2048.0
    mid = r1.to(torch.float16)
    lo = ((r1 - mid.to(torch.float32)) * 2048.0).to(torch.float16)
    return hi.contiguous(), mid.contiguous(), lo.contiguous()


def split_weights3_many(weights):
    """split_weights3 of several conv weights with the elementwise work of equally shaped ones
    done on one stacked tensor (a training loop re-splits all 7 blocks after every update)."""
    out = [None] * len(weights)
    groups = {}
    for i, w in enumerate(weights):
        groups.setdefault(tuple(w.shape), []).append(i)
    for shape, idx in groups.items():
        cout, cin, kh, kw = shape
        if (kh, kw) != (3, 3) or cin % 16 or cout != 128:
            raise ValueError("split_weights3: need (128, 16k, 3, 3) weights")
        w = torch.stack([weights[i].detach().to(torch.float32) for i in idx])          # L, co, ci, ky, kx
        w = w.permute(0, 3, 4, 1, 2).reshape(len(idx), 3, 3, cout, cin // 16, 16).permute(0, 4, 1, 2, 3, 5).contiguous()
        hi = w.to(torch.float16)
        r1 = (w - hi.to(torch.float32)) * 2048.0
        mid = r1.to(torch.float16)
        lo = ((r1 - mid.to(torch.float32)) * 2048.0).to(torch.float16)
        for j, i in enumerate(idx):
            out[i] = (hi[j], mid[j], lo[j])
    return out


POLICY_SCRATCH_ROW_BYTES = 51200   # a board's LDS image in iago_policy_forward_split3 (64 rows of 800 B)


def policy_split3_prepare(w1, b1, layers, w9, b10):
    """The weight half of iago_policy_split3_args, checked once: a template that
    policy_forward_split3_prepared copies per call.  The caller keeps the tensors alive."""
    a = _lib.PolicySplit3Args()
    if len(layers) != 7 or tuple(w1.shape) != (64, 2, 3, 3) or w9.numel() != 128 or b10.numel() != 64:
        raise ValueError("policy_forward_split3: unexpected shapes")
    a.w1, a.b1 = _dev(w1, torch.float32, "w1").value, _dev(b1, torch.float32, "b1").value
    for k, (w_hi, w_mid, w_lo, bias) in enumerate(layers):
        if w_hi.shape != ((4 if k == 0 else 8), 3, 3, 128, 16):
            raise ValueError("policy_forward_split3: layer %d: weight blocks %s" % (k, tuple(w_hi.shape)))
        a.w_hi[k] = _dev(w_hi, torch.float16, "w_hi").value
        a.w_mid[k] = _dev(w_mid, torch.float16, "w_mid").value
        a.w_lo[k] = _dev(w_lo, torch.float16, "w_lo").value
        a.bias[k] = _dev(bias, torch.float32, "bias").value
    a.w9 = _dev(w9.reshape(128), torch.float32, "w9").value
    a.b10 = _dev(b10, torch.float32, "b10").value
    return a


def policy_forward_split3_prepared(template, own, opp, n=None, index=None, n_dev=None, overflow=None, parts=1,
                                   scratch=None):
    """policy_forward_split3 with the weights of policy_split3_prepare."""
    a = _lib.PolicySplit3Args.from_buffer_copy(template)
    n = own.numel() if n is None else n
    if index is not None:
        n = min(n, index.numel())
        a.index = _dev(index, torch.int64, "index").value
    if n_dev is not None:
        a.n_dev = _dev(n_dev, torch.int32, "n_dev").value
    a.own, a.opp = _dev(own, torch.int64, "own").value, _dev(opp, torch.int64, "opp").value
    a.n = n
    probs = torch.empty((n, 64), dtype=torch.float32, device=own.device)
    a.probs = probs.data_ptr()
    if parts > 1:
        _set_scratch(a, parts, scratch, n)
    f = _flag(overflow)
    a.overflow = f.value if f is not None else None
    check(_lib.lib().iago_policy_forward_split3(C.byref(a), _stream()), "iago_policy_forward_split3")
    return probs


def _set_scratch(a, parts, scratch, n):
    """parts > 1: scratch = uint8 [rows][POLICY_SCRATCH_ROW_BYTES]; a batch of more than `rows`
    rows runs as chunks of `rows` (iago_policy_split3_args.scratch_rows)."""
    rows = 0 if scratch is None else scratch.numel() // POLICY_SCRATCH_ROW_BYTES
    if rows < 1:
        raise ValueError("policy_forward_split3: parts > 1 needs a scratch buffer of (rows, %d) bytes"
                         % POLICY_SCRATCH_ROW_BYTES)
    a.parts, a.scratch = parts, _dev(scratch, torch.uint8, "scratch").value
    a.scratch_rows = min(rows, n, 0x7FFFFFFF)


def policy_forward_split3(own, opp, w1, b1, layers, w9, b10, n=None, index=None, n_dev=None, overflow=None,
                          parts=1, scratch=None):
    """The whole SLPolicy net in one launch (iago_policy_forward_split3): boards (own = side to
    move) -> (n, 64) probabilities.  layers: the 7 (w_hi, w_mid, w_lo, bias) of blocks 2..8
    (split_weights3); index / n_dev: optional device-side gather list and row count."""
    a = _lib.PolicySplit3Args()
    n = own.numel() if n is None else n
    if index is not None:
        n = min(n, index.numel())
        a.index = _dev(index, torch.int64, "index").value
    if n_dev is not None:
        a.n_dev = _dev(n_dev, torch.int32, "n_dev").value
    if len(layers) != 7 or tuple(w1.shape) != (64, 2, 3, 3) or w9.numel() != 128 or b10.numel() != 64:
        raise ValueError("policy_forward_split3: unexpected shapes")
    a.own, a.opp = _dev(own, torch.int64, "own").value, _dev(opp, torch.int64, "opp").value
    a.n = n
    a.w1, a.b1 = _dev(w1, torch.float32, "w1").value, _dev(b1, torch.float32, "b1").value
    for k, (w_hi, w_mid, w_lo, bias) in enumerate(layers):
        if w_hi.shape != ((4 if k == 0 else 8), 3, 3, 128, 16):
            raise ValueError("policy_forward_split3: layer %d: weight blocks %s" % (k, tuple(w_hi.shape)))
        a.w_hi[k] = _dev(w_hi, torch.float16, "w_hi").value
        a.w_mid[k] = _dev(w_mid, torch.float16, "w_mid").value
        a.w_lo[k] = _dev(w_lo, torch.float16, "w_lo").value
        a.bias[k] = _dev(bias, torch.float32, "bias").value
    a.w9 = _dev(w9.reshape(128), torch.float32, "w9").value
    a.b10 = _dev(b10, torch.float32, "b10").value
    probs = torch.empty((n, 64), dtype=torch.float32, device=own.device)
    a.probs = probs.data_ptr()
    if parts > 1:
        # parts launches (per chunk of the scratch's rows); scratch not shared with a call on
        # another stream (the launches of a call, and the calls of a stream, run in order)
        _set_scratch(a, parts, scratch, n)
    f = _flag(overflow)
    a.overflow = f.value if f is not None else None
    check(_lib.lib().iago_policy_forward_split3(C.byref(a), _stream()), "iago_policy_forward_split3")
    return probs


def split_head_weights(w9):
    """Value.block9's (1, 128, 3, 3) weight as the MFMA operand of iago_value_forward_split:
    (hi, lo) f16 [8 chunks][32 rows][16], row r < 9 = kernel tap r, the other rows zero."""
    if tuple(w9.shape) != (1, 128, 3, 3):
        raise ValueError("split_head_weights: (1, 128, 3, 3) expected")
    w = w9.detach().to(torch.float32).reshape(8, 16, 9).permute(0, 2, 1)   # chunk, tap, channel
    a = torch.zeros((8, 32, 16), dtype=torch.float32, device=w9.device)
    a[:, :9, :] = w
    hi = a.to(torch.float16)
    lo = ((a - hi.to(torch.float32)) * 2048.0).to(torch.float16)
    return hi.contiguous(), lo.contiguous()


def value_split_weights(a, w1, b1, layers, head, b9, w10, w11):
    """The weight half of an iago_value_split_args, checked (value_forward_split, the persistent search)."""
    if len(layers) != 7 or tuple(w1.shape) != (64, 2, 3, 3) or tuple(w10.shape) != (128, 64) \
            or tuple(w11.shape) != (1, 128):
        raise ValueError("value_forward_split: unexpected shapes")
    a.w1, a.b1 = _dev(w1, torch.float32, "w1").value, _dev(b1, torch.float32, "b1").value
    for k, (w_hi, w_lo, bias) in enumerate(layers):
        if w_hi.shape != ((4 if k == 0 else 8), 3, 3, 128, 16):
            raise ValueError("value_forward_split: layer %d: weight blocks %s" % (k, tuple(w_hi.shape)))
        a.w_hi[k] = _dev(w_hi, torch.float16, "w_hi").value
        a.w_lo[k] = _dev(w_lo, torch.float16, "w_lo").value
        a.bias[k] = _dev(bias, torch.float32, "bias").value
    a.w9_hi, a.w9_lo = _dev(head[0], torch.float16, "w9_hi").value, _dev(head[1], torch.float16, "w9_lo").value
    a.b9 = _dev(b9, torch.float32, "b9").value
    a.w10, a.w11 = _dev(w10, torch.float32, "w10").value, _dev(w11, torch.float32, "w11").value


def value_forward_split(x, w1, b1, layers, head, w9, b9, w10, w11, overflow=None, index=None, n_dev=None,
                        out=None, rollout=None, async_ref=None, batch=None):
    """The whole Value net in one launch (iago_value_forward_split).  x: float32 planes
    (n, 2, 8, 8) or a pair (own, opp) of int64 bitboards (own = side to move); layers: the 7
    (w_hi, w_lo, bias) of blocks 2..8 (split_weights); head: split_head_weights(w9).
    index / n_dev (boards only): evaluate boards index[0 .. min(n, *n_dev)) and write their
    values to out[index[i]] (out: (n_boards,) float32, the other entries untouched).
    rollout: a PreparedRollout (rollout_prepare) to play in the SAME launch (iago_value_rollout:
    the leaf evaluation of a playout, value net on the listed leaves + rollout of all).
    batch = (boards per workgroup, max workgroups): the device-counted batch form for work off the
    playouts' critical path (iago_value_forward_batch; n_dev required)."""
    a = _lib.ValueSplitArgs()
    if isinstance(x, tuple):
        own, opp = x
        n, dev = own.numel(), own.device
        a.own, a.opp = _dev(own, torch.int64, "own").value, _dev(opp, torch.int64, "opp").value
    else:
        if tuple(x.shape[1:]) != (2, 8, 8):
            raise ValueError("value_forward_split: planes (n, 2, 8, 8) expected")
        n, dev = x.shape[0], x.device
        a.planes = _dev(x, torch.float32, "planes").value
    a.n = n
    value_split_weights(a, w1, b1, layers, head, b9, w10, w11)
    if index is not None:
        if not isinstance(x, tuple) or out is None:
            raise ValueError("value_forward_split: a gather list needs (own, opp) boards and an `out` buffer")
        n = min(index.numel(), n)
        a.n = n
        a.index = _dev(index, torch.int64, "index").value
    if n_dev is not None:
        a.n_dev = _dev(n_dev, torch.int32, "n_dev").value
    if out is None:
        out = torch.empty((n,), dtype=torch.float32, device=dev)
    a.out = _dev(out, torch.float32, "out").value
    f = _flag(overflow)
    a.overflow = f.value if f is not None else None
    if async_ref is not None:
        # one game-asynchronous step's leaf evaluation: the rollouts of the games that descended and
        # one piece of the value net for every queue of fresh leaves (iago_value_rollout_async)
        check(_lib.lib().iago_value_rollout_async(C.byref(a), rollout.ref, async_ref, _stream()),
              "iago_value_rollout_async")
    elif rollout is not None:
        check(_lib.lib().iago_value_rollout(C.byref(a), rollout.ref, _stream()), "iago_value_rollout")
    elif batch is not None:
        check(_lib.lib().iago_value_forward_batch(C.byref(a), int(batch[0]), int(batch[1]), _stream()),
              "iago_value_forward_batch")
    else:
        check(_lib.lib().iago_value_forward_split(C.byref(a), _stream()), "iago_value_forward_split")
    return out


def conv3x3_split(a, w_hi, w_lo, bias, overflow=None):
    """relu(conv3x3(a, w) + bias) on SplitActs: Block.__call__ (network.py:9-13) on
    the MFMA units in split-f16 arithmetic.  w_hi, w_lo from split_weights."""
    cin = a.channels
    if w_hi.shape != (cin // 16, 3, 3, 128, 16):
        raise ValueError("weight blocks %s do not match %d input channels" % (tuple(w_hi.shape), cin))
    hi = torch.empty((a.n, 8, 64, 16), dtype=torch.float16, device=a.hi.device)
    lo = torch.empty_like(hi)
    check(_lib.lib().iago_conv3x3_split(_dev(a.hi, torch.float16, "x_hi"), _dev(a.lo, torch.float16, "x_lo"),
                                        _dev(w_hi, torch.float16, "w_hi"), _dev(w_lo, torch.float16, "w_lo"),
                                        _dev(bias, torch.float32, "bias"),
                                        _dev(hi, torch.float16, "y_hi"), _dev(lo, torch.float16, "y_lo"),
                                        a.n, cin, 128, _flag(overflow), _stream()), "iago_conv3x3_split")
    return SplitActs(hi, lo, 128)


# ---- gradients of the REINFORCE update in split-f16 arithmetic (csrc/policy_grad_kernels.hip) ----

WGRAD_GROUPS = 32   # groups of boards whose partial weight gradients are summed in order (a multiple of 8)


def conv3x3_wgrad_split(dy, x, scale_exp=None, groups=WGRAD_GROUPS, part=None):
    """Weight gradient of one 3x3 block: dy, x SplitActs (dy: 128 channels, times 2**scale_exp), returns
    dW (128, cin, 3, 3) float32 (include/iago_hip.h)."""
    cin = x.channels
    if dy.channels != 128 or dy.n != x.n:
        raise ValueError("conv3x3_wgrad_split: dy must be (n, 128) channels on the rows of x")
    if part is None:
        part = torch.empty((groups, 9, 128, cin), dtype=torch.float32, device=x.hi.device)
    dw = torch.empty((128, cin, 3, 3), dtype=torch.float32, device=x.hi.device)
    check(_lib.lib().iago_conv3x3_wgrad_split(_dev(dy.hi, torch.float16, "dy_hi"), _dev(dy.lo, torch.float16, "dy_lo"),
                                              _dev(x.hi, torch.float16, "x_hi"), _dev(x.lo, torch.float16, "x_lo"),
                                              x.n, cin, _dev(part, torch.float32, "part"), groups,
                                              _dev(scale_exp, torch.int32, "scale_exp") if scale_exp is not None else None,
                                              _dev(dw, torch.float32, "dw"), _stream()), "iago_conv3x3_wgrad_split")
    return dw


def split_weights_transposed(weight):
    """The backward-data form of a (128, cin, 3, 3) block weight: split_weights of Wt[ci][co][ky][kx] =
    W[co][ci][2-ky][2-kx], padded to 128 rows."""
    cout, cin = weight.shape[0], weight.shape[1]
    wt = weight.detach().to(torch.float32).flip(2, 3).permute(1, 0, 2, 3)
    if cin < 128:
        wt = torch.cat([wt, torch.zeros((128 - cin, cout, 3, 3), dtype=torch.float32, device=wt.device)])
    return split_weights(wt.contiguous())


def split_weights_transposed_many(weights):
    """split_weights_transposed of several block weights, the elementwise work of equally shaped ones on one stacked
    tensor (the update re-splits all 7 blocks after every step)."""
    out = [None] * len(weights)
    groups = {}
    for i, w in enumerate(weights):
        groups.setdefault(tuple(w.shape), []).append(i)
    for shape, idx in groups.items():
        cout, cin, kh, kw = shape
        if (kh, kw) != (3, 3) or cout != 128 or cin not in (64, 128):
            raise ValueError("split_weights_transposed: need (128, 64|128, 3, 3) weights")
        w = torch.stack([weights[i].detach().to(torch.float32) for i in idx])            # L, co, ci, ky, kx
        wt = w.flip(3, 4).permute(0, 3, 4, 2, 1)                                          # L, ky', kx', ci, co
        if cin < 128:
            wt = torch.cat([wt, torch.zeros((len(idx), 3, 3, 128 - cin, cout), dtype=torch.float32, device=w.device)], 3)
        wt = wt.reshape(len(idx), 3, 3, 128, cout // 16, 16).permute(0, 4, 1, 2, 3, 5).contiguous()
        hi = wt.to(torch.float16)
        lo = ((wt - hi.to(torch.float32)) * 2048.0).to(torch.float16)
        for j, i in enumerate(idx):
            out[i] = (hi[j], lo[j])
    return out


def adam_chainer(params, grads, ms, vs, alpha_t, beta1, beta2, eps, weight_decay, steps=None):
    """iago_adam_chainer: one launch for all (float32, contiguous, CUDA) parameters; m / v in place, the parameters
    too unless `steps` (tensors that receive alpha_t m / (sqrt(v) + eps), for the caller to subtract) is given."""
    if len(params) > _lib.ADAM_MAX_TENSORS:
        raise ValueError("adam_chainer: at most %d tensors" % _lib.ADAM_MAX_TENSORS)
    A = _lib.AdamArgs()
    for k, (p, g, m, v) in enumerate(zip(params, grads, ms, vs)):
        A.p[k], A.g[k] = _dev(p, torch.float32, "p").value, _dev(g, torch.float32, "g").value
        A.m[k], A.v[k] = _dev(m, torch.float32, "m").value, _dev(v, torch.float32, "v").value
        A.count[k] = p.numel()
        if steps is not None:
            A.step[k] = _dev(steps[k], torch.float32, "step").value
    A.n_tensors = len(params)
    A.alpha_t, A.one_minus_beta1, A.one_minus_beta2 = alpha_t, 1.0 - beta1, 1.0 - beta2
    A.eps, A.weight_decay = eps, weight_decay
    check(_lib.lib().iago_adam_chainer(C.byref(A), _stream()), "iago_adam_chainer")


_grad_workspace = {}


def _grad_workspace_at_least(device, need):
    """The one scratch buffer of the gradient entry points on `device` (iago_policy_reinforce_grad,
    iago_value_mse_grad): kept between calls, grown to the largest need seen."""
    ws = _grad_workspace.get(str(device))
    if ws is None or ws.numel() < need:
        _grad_workspace[str(device)] = ws = None      # (release before the larger allocation)
        ws = torch.empty(need, dtype=torch.uint8, device=device)
        _grad_workspace[str(device)] = ws
    return ws


def policy_grad_workspace(device, n):
    """The scratch of iago_policy_reinforce_grad for n rows on `device`: kept, grown in steps of 256 rows."""
    return _grad_workspace_at_least(device, int(_lib.lib().iago_policy_grad_workspace_bytes((n + 255) // 256 * 256)))


def value_grad_workspace(device, n):
    """The scratch of iago_value_mse_grad for n rows on `device`: the same buffer as policy_grad_workspace's."""
    return _grad_workspace_at_least(device, int(_lib.lib().iago_value_grad_workspace_bytes((n + 255) // 256 * 256)))


def release_grad_workspace():
    """Free the scratch policy_grad_workspace / value_grad_workspace keep (308 KB per row of the largest batch seen
    + 247 MB)."""
    _grad_workspace.clear()


def _policy_grad_common(A, own, opp, n_mean, w1, b1, layers, layers_t, w9, b10, grads, probs, overflow):
    """The fields iago_policy_grad_args and iago_policy_visits_grad_args share.  Returns the loss's device word."""
    n = own.numel()
    dev = own.device
    ws = policy_grad_workspace(dev, n)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    A.own, A.opp = _dev(own, torch.int64, "own"), _dev(opp, torch.int64, "opp")
    A.n, A.n_mean = n, int(n_mean)
    A.w1, A.b1 = _dev(w1, torch.float32, "w1"), _dev(b1, torch.float32, "b1")
    for k in range(7):
        A.w_hi[k], A.w_lo[k] = _dev(layers[k][0], torch.float16, "w_hi").value, _dev(layers[k][1], torch.float16, "w_lo").value
        A.bias[k] = _dev(layers[k][2], torch.float32, "bias").value
        A.wt_hi[k], A.wt_lo[k] = (_dev(layers_t[k][0], torch.float16, "wt_hi").value,
                                  _dev(layers_t[k][1], torch.float16, "wt_lo").value)
        A.g_w[k], A.g_b[k] = _dev(grads["w"][k], torch.float32, "g_w").value, _dev(grads["b"][k], torch.float32, "g_b").value
    A.w9, A.b10 = _dev(w9, torch.float32, "w9"), _dev(b10, torch.float32, "b10")
    A.g_w1, A.g_b1 = _dev(grads["w1"], torch.float32, "g_w1"), _dev(grads["b1"], torch.float32, "g_b1")
    A.g_w9, A.g_b10 = _dev(grads["w9"], torch.float32, "g_w9"), _dev(grads["b10"], torch.float32, "g_b10")
    A.loss = _dev(loss, torch.float32, "loss")
    A.probs = _dev(probs, torch.float32, "probs") if probs is not None else None
    A.workspace, A.workspace_bytes = ws.data_ptr(), ws.numel()
    A.overflow = _flag(overflow)
    return loss


def policy_reinforce_grad(own, opp, action, reward, n_mean, w1, b1, layers, layers_t, w9, b10, grads, probs=None,
                          overflow=None):
    """iago_policy_reinforce_grad (include/iago_hip.h): the gradients of mean(softmax_cross_entropy(model(x), a) * r)
    (src/train_rl.py:61-65) written to `grads` = dict(w1, b1, w=[7], b=[7], w9, b10) of float32 tensors in the
    parameters' shapes.  layers: 7 x (w_hi, w_lo, bias) as for conv3x3_split; layers_t: 7 x (wt_hi, wt_lo) from
    split_weights_transposed.  Returns the loss (0-dim float32 device tensor)."""
    A = _lib.PolicyGradArgs()
    loss = _policy_grad_common(A, own, opp, n_mean, w1, b1, layers, layers_t, w9, b10, grads, probs, overflow)
    A.action, A.reward = _dev(action, torch.int32, "action"), _dev(reward, torch.float32, "reward")
    check(_lib.lib().iago_policy_reinforce_grad(C.byref(A), _stream()), "iago_policy_reinforce_grad")
    return loss


def policy_visits_grad(own, opp, visits, weight, n_mean, w1, b1, layers, layers_t, w9, b10, grads, probs=None,
                       overflow=None):
    """iago_policy_visits_grad (include/iago_hip_training.h): the gradients of the cross-entropy of model(x) against
    the rows' visit distributions visits / sum(visits), weighted per row, summed and divided by n_mean; written to
    `grads` as policy_reinforce_grad writes them (the same layers, layers_t).  visits: (n, 64) int32, >= 0 (a negative
    count raises bit 1 of `overflow`); weight: (n,) float32 or None (1 for every row).  Returns the loss (0-dim float32
    device tensor)."""
    n = own.numel()
    if visits.dtype != torch.int32 or tuple(visits.shape) != (n, 64):
        raise ValueError("policy_visits_grad: visits must be int32 (n, 64)")
    if weight is not None and tuple(weight.shape) != (n,):
        raise ValueError("policy_visits_grad: weight must be (n,)")
    A = _lib.PolicyVisitsGradArgs()
    loss = _policy_grad_common(A, own, opp, n_mean, w1, b1, layers, layers_t, w9, b10, grads, probs, overflow)
    A.visits = _dev(visits, torch.int32, "visits")
    A.weight = _dev(weight, torch.float32, "weight") if weight is not None else None
    check(_lib.lib().iago_policy_visits_grad(C.byref(A), _stream()), "iago_policy_visits_grad")
    return loss


DROPOUT_SCALE = float(np.float32(1.0 / (1.0 - 0.4)))   # F.dropout(h, 0.4)'s factor of the kept units, float32


def value_mse_grad(own, opp, result, n_mean, w1, b1, layers, layers_t, w9, b9, w10, w11, grads, keep=None,
                   dropout_scale=DROPOUT_SCALE, pred=None, h9=None, overflow=None):
    """iago_value_mse_grad (include/iago_hip_training.h): the gradients of sum((Value(x) - result)^2) / n_mean
    (train_value.py:53-57) written to `grads` = dict(w1, b1, w=[7], b=[7], w9, b9, w10, w11) of float32 tensors in
    the parameters' shapes.  layers: 7 x (w_hi, w_lo, bias) as for conv3x3_split; layers_t: 7 x (wt_hi, wt_lo) from
    split_weights_transposed.  keep: optional (n, 128) mask of fc10's units (nonzero = kept, scaled by
    dropout_scale); None = no dropout.  pred (n,) / h9 (n, 64): optional float32 outputs.  Returns the loss (0-dim
    float32 device tensor)."""
    n = own.numel()
    dev = own.device
    ws = value_grad_workspace(dev, n)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    A = _lib.ValueGradArgs()
    A.own, A.opp = _dev(own, torch.int64, "own"), _dev(opp, torch.int64, "opp")
    A.result = _dev(result, torch.float32, "result")
    if keep is not None:
        if tuple(keep.shape) != (n, 128):
            raise ValueError("value_mse_grad: keep must be (n, 128)")
        A.keep = _dev(keep, torch.uint8, "keep")
    A.dropout_scale = dropout_scale
    A.n, A.n_mean = n, int(n_mean)
    A.w1, A.b1 = _dev(w1, torch.float32, "w1"), _dev(b1, torch.float32, "b1")
    for k in range(7):
        A.w_hi[k], A.w_lo[k] = _dev(layers[k][0], torch.float16, "w_hi").value, _dev(layers[k][1], torch.float16, "w_lo").value
        A.bias[k] = _dev(layers[k][2], torch.float32, "bias").value
        A.wt_hi[k], A.wt_lo[k] = (_dev(layers_t[k][0], torch.float16, "wt_hi").value,
                                  _dev(layers_t[k][1], torch.float16, "wt_lo").value)
        A.g_w[k], A.g_b[k] = _dev(grads["w"][k], torch.float32, "g_w").value, _dev(grads["b"][k], torch.float32, "g_b").value
    A.w9, A.b9 = _dev(w9, torch.float32, "w9"), _dev(b9, torch.float32, "b9")
    A.w10, A.w11 = _dev(w10, torch.float32, "w10"), _dev(w11, torch.float32, "w11")
    A.g_w1, A.g_b1 = _dev(grads["w1"], torch.float32, "g_w1"), _dev(grads["b1"], torch.float32, "g_b1")
    A.g_w9, A.g_b9 = _dev(grads["w9"], torch.float32, "g_w9"), _dev(grads["b9"], torch.float32, "g_b9")
    A.g_w10, A.g_w11 = _dev(grads["w10"], torch.float32, "g_w10"), _dev(grads["w11"], torch.float32, "g_w11")
    A.loss = _dev(loss, torch.float32, "loss")
    A.pred = _dev(pred, torch.float32, "pred") if pred is not None else None
    A.h9 = _dev(h9, torch.float32, "h9") if h9 is not None else None
    A.workspace, A.workspace_bytes = ws.data_ptr(), ws.numel()
    A.overflow = _flag(overflow)
    check(_lib.lib().iago_value_mse_grad(C.byref(A), _stream()), "iago_value_mse_grad")
    return loss


def conv3x3_bwd_data_split(dy, scale_exp, wt_hi, wt_lo, saved, max_bits=None):
    """Gradient at a block's input through the ReLU of the block below (saved: its SplitActs output).  Returns
    (dx float32 (n, C/16, 64, 16), max_bits)."""
    n, ch = dy.n, saved.channels
    dx = torch.empty((n, ch // 16, 64, 16), dtype=torch.float32, device=dy.hi.device)
    if max_bits is None:
        max_bits = torch.zeros(1, dtype=torch.int32, device=dy.hi.device)
    check(_lib.lib().iago_conv3x3_bwd_data_split(_dev(dy.hi, torch.float16, "dy_hi"), _dev(dy.lo, torch.float16, "dy_lo"),
                                                 _dev(scale_exp, torch.int32, "scale_exp"),
                                                 _dev(wt_hi, torch.float16, "wt_hi"), _dev(wt_lo, torch.float16, "wt_lo"),
                                                 _dev(saved.hi, torch.float16, "mask_hi"), _dev(saved.lo, torch.float16, "mask_lo"),
                                                 ch, _dev(dx, torch.float32, "dx"), _dev(max_bits, torch.int32, "max_bits"),
                                                 n, _stream()), "iago_conv3x3_bwd_data_split")
    return dx, max_bits


def split_scaled(x, max_bits, bias_grad=False):
    """float32 channel blocks (n, C/16, 64, 16) -> (SplitActs of x * 2**e, e as an int32 device word[, the sums
    over boards and cells per channel])."""
    n, nb = x.shape[0], x.shape[1]
    hi = torch.empty((n, nb, 64, 16), dtype=torch.float16, device=x.device)
    lo = torch.empty_like(hi)
    e = torch.empty(1, dtype=torch.int32, device=x.device)
    part = db = None
    if bias_grad:
        part = torch.empty(((n * nb + 1) // 2) * 32, dtype=torch.float32, device=x.device)
        db = torch.empty(nb * 16, dtype=torch.float32, device=x.device)
    check(_lib.lib().iago_split_scaled(_dev(x, torch.float32, "x"), _dev(max_bits, torch.int32, "max_bits"),
                                       _dev(hi, torch.float16, "hi"), _dev(lo, torch.float16, "lo"),
                                       _dev(e, torch.int32, "scale_exp"), n, nb * 16,
                                       _dev(part, torch.float32, "bias_part") if bias_grad else None,
                                       _dev(db, torch.float32, "bias_grad") if bias_grad else None,
                                       _stream()), "iago_split_scaled")
    return (SplitActs(hi, lo, nb * 16), e, db) if bias_grad else (SplitActs(hi, lo, nb * 16), e)


def blocks_to_nchw(x):
    """float32 channel blocks (n, C/16, 64, 16) -> (n, C, 8, 8)."""
    n, nb = x.shape[0], x.shape[1]
    return x.permute(0, 1, 3, 2).reshape(n, nb * 16, 8, 8)


def nchw_to_blocks(x):
    """(n, C, 8, 8) float32 -> channel blocks (n, C/16, 64, 16)."""
    n, c = x.shape[0], x.shape[1]
    return x.reshape(n, c // 16, 16, 64).permute(0, 1, 3, 2).contiguous()


# ---- float32 small-batch convolution stack (policy net on expansions) ----------------

def f32_weights(weight):
    """(128, cin, 3, 3) float32 conv weight -> [4][9][cin][32] as iago_conv3x3_f32 reads it."""
    cout, cin, kh, kw = weight.shape
    if (kh, kw) != (3, 3) or cout != 128 or cin not in (64, 128):
        raise ValueError("f32_weights: need a (128, 64|128, 3, 3) weight")
    w = weight.detach().to(torch.float32).permute(2, 3, 1, 0).reshape(9, cin, 4, 32)
    return w.permute(2, 0, 1, 3).contiguous()


def conv3x3_f32(x, w4, bias, n_dev=None):
    """relu(conv3x3(x, w) + bias) in float32 on the matrix units; x (n, cin, 8, 8)."""
    n, cin = x.shape[0], x.shape[1]
    if tuple(w4.shape) != (4, 9, cin, 32):
        raise ValueError("weight layout %s does not match %d input channels" % (tuple(w4.shape), cin))
    y = torch.empty((n, 128, 8, 8), dtype=torch.float32, device=x.device)
    check(_lib.lib().iago_conv3x3_f32(_dev(x, torch.float32, "x"), _dev(w4, torch.float32, "w"),
                                      _dev(bias, torch.float32, "bias"), _dev(y, torch.float32, "y"),
                                      n, cin, 128, _count(n_dev), _stream()), "iago_conv3x3_f32")
    return y


def stem_f32(planes, w1, b1, n_dev=None):
    n = planes.shape[0]
    if tuple(planes.shape[1:]) != (2, 8, 8) or tuple(w1.shape) != (64, 2, 3, 3):
        raise ValueError("stem_f32: planes (n,2,8,8) and w1 (64,2,3,3) expected")
    y = torch.empty((n, 64, 8, 8), dtype=torch.float32, device=planes.device)
    check(_lib.lib().iago_stem_f32(_dev(planes, torch.float32, "planes"), _dev(w1, torch.float32, "w1"),
                                   _dev(b1, torch.float32, "b1"), _dev(y, torch.float32, "y"), n,
                                   _count(n_dev), _stream()), "iago_stem_f32")
    return y


def stem_f32_boards(own, opp, index, w1, b1, n, n_dev=None):
    """stem_f32 of boards index[0..n) (int64 tensor or None = the first n boards) without the
    planes tensor; own = side to move."""
    if tuple(w1.shape) != (64, 2, 3, 3):
        raise ValueError("stem_f32_boards: w1 (64,2,3,3) expected")
    if index is not None and index.numel() < n:
        raise ValueError("index is shorter than n")
    y = torch.empty((n, 64, 8, 8), dtype=torch.float32, device=own.device)
    check(_lib.lib().iago_stem_f32_boards(_dev(own, torch.int64, "own"), _dev(opp, torch.int64, "opp"),
                                          _dev(index, torch.int64, "index") if index is not None else None,
                                          _dev(w1, torch.float32, "w1"), _dev(b1, torch.float32, "b1"),
                                          _dev(y, torch.float32, "y"), n, _count(n_dev), _stream()),
          "iago_stem_f32_boards")
    return y


def policy_head(x, w9, b10, n_dev=None):
    """softmax(conv1x1(x, w9) + b10) (network.py:29-47): x (n, 128, 8, 8) -> (n, 64)."""
    n = x.shape[0]
    if tuple(x.shape[1:]) != (128, 8, 8) or w9.numel() != 128 or b10.numel() != 64:
        raise ValueError("policy_head: unexpected shapes")
    probs = torch.empty((n, 64), dtype=torch.float32, device=x.device)
    check(_lib.lib().iago_policy_head(_dev(x, torch.float32, "x"), _dev(w9.reshape(128), torch.float32, "w9"),
                                      _dev(b10, torch.float32, "b10"), _dev(probs, torch.float32, "probs"),
                                      n, _count(n_dev), _stream()), "iago_policy_head")
    return probs


def sample_moves(probs, legal, uniforms=None, seed=0, id_base=0, step=0, stream_id=0):
    """Masked inverse-CDF sampling (src/rl_self_play.py:111-122); int8 actions,
    -1 where there is no legal move.  uniforms: optional float64 (n,)."""
    n = legal.numel()
    if probs.numel() != n * 64:
        raise ValueError("probs must be (n, 64)")
    out = torch.empty(n, dtype=torch.int8, device=legal.device)
    up = _dev(uniforms, torch.float64, "uniforms") if uniforms is not None else None
    check(_lib.lib().iago_sample_moves(_dev(probs, torch.float32, "probs"),
                                       _dev(legal, torch.int64, "legal"), up,
                                       int(seed) & 0xFFFFFFFFFFFFFFFF, int(id_base) & 0xFFFFFFFF,
                                       int(step) & 0xFFFFFFFF, int(stream_id) & 0xFFFFFFFF,
                                       _dev(out, torch.int8, "action"), n, _stream()),
          "iago_sample_moves")
    return out


class RolloutWeights(object):
    """Device-resident RolloutPolicy parameters (network.py:49-64) in the form
    the rollout kernel consumes (the table blob of iago_rollout_build_table).
    w = None builds the uniform policy."""

    def __init__(self, w=None, b=None, device="cuda"):
        blob = np.empty(IAGO_ROLLOUT_TABLE_FLOATS, dtype=np.float32)
        if w is None:
            self.w = self.b = None
            wp = bp = None
        else:
            self.w = np.ascontiguousarray(np.asarray(w, dtype=np.float32).reshape(18))
            self.b = np.ascontiguousarray(np.asarray(b, dtype=np.float32).reshape(64))
            wp, bp = C.c_void_p(self.w.ctypes.data), C.c_void_p(self.b.ctypes.data)
        check(_lib.lib().iago_rollout_build_table(wp, bp, C.c_void_p(blob.ctypes.data)),
              "iago_rollout_build_table")
        self.log_form = 0 if blob[_lib.ROLLOUT_MODE_INDEX] == 1.0 else 1
        self.table = torch.from_numpy(blob).to(device)


_UNIFORM = {}


def uniform_weights(device="cuda"):
    key = str(device)
    if key not in _UNIFORM:
        _UNIFORM[key] = RolloutWeights(None, None, device)
    return _UNIFORM[key]


class RolloutResult(object):
    __slots__ = ("z", "final_own", "final_opp", "n_turns", "trace")

    def __init__(self):
        self.z = self.final_own = self.final_opp = self.n_turns = self.trace = None


class PreparedRollout(object):
    """A fully marshalled iago_rollout call: `launch(stream)` costs one ctypes
    call.  Holds references to every tensor the launch touches."""
    __slots__ = ("args", "ref", "result", "_keep", "_fn")

    def launch(self, stream_ptr=None):
        """Enqueue on `stream_ptr` (a hipStream_t as int / c_void_p; None =
        torch's current stream); returns the iago status code."""
        if stream_ptr is None:
            stream_ptr = _stream()
        return self._fn(self.ref, stream_ptr)


def rollout_prepare(own, opp, weights=None, seed=0, id_base=0, stream_id=0, uniforms=None,
                    want_final=False, want_turns=False, want_trace=False, out=None,
                    throughput_hint=False, stream_id_dev=None):
    """Marshal a rollout launch once (see `rollout` for the arguments)."""
    n = own.numel()
    res = out if out is not None else RolloutResult()
    dev = own.device
    if res.z is None:
        res.z = torch.empty(n, dtype=torch.int8, device=dev)
    if want_final and res.final_own is None:
        res.final_own = torch.empty(n, dtype=torch.int64, device=dev)
        res.final_opp = torch.empty(n, dtype=torch.int64, device=dev)
    if want_turns and res.n_turns is None:
        res.n_turns = torch.empty(n, dtype=torch.uint8, device=dev)
    if want_trace and res.trace is None:
        res.trace = torch.full((IAGO_MAX_TURNS, n), 0xFE, dtype=torch.uint8, device=dev)
    if weights is None:
        weights = uniform_weights(dev)
    a = RolloutArgs()
    a.own = _dev(own, torch.int64, "own")
    a.opp = _dev(opp, torch.int64, "opp")
    a.n = n
    a.table = _dev(weights.table, torch.float32, "table")
    a.log_form = weights.log_form
    a.throughput_hint = int(throughput_hint)  # False / 0: automatic, True / 1: lane per board, 2: 8 lanes per board
    if uniforms is not None:
        if tuple(uniforms.shape) != (IAGO_MAX_TURNS, n):
            raise ValueError("uniforms must have shape (%d, n)" % IAGO_MAX_TURNS)
        a.uniforms = _dev(uniforms, torch.float32, "uniforms")
    a.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    a.id_base = int(id_base) & 0xFFFFFFFF
    a.stream_id = int(stream_id) & 0xFFFFFFFF
    if stream_id_dev is not None:  # int32 CUDA tensor with one element, added on the device
        a.stream_id_dev = _dev(stream_id_dev, torch.int32, "stream_id_dev")
    a.z = _dev(res.z, torch.int8, "z")
    if res.final_own is not None:
        a.final_own = _dev(res.final_own, torch.int64, "final_own")
        a.final_opp = _dev(res.final_opp, torch.int64, "final_opp")
    if res.n_turns is not None:
        a.n_turns = _dev(res.n_turns, torch.uint8, "n_turns")
    if res.trace is not None:
        a.trace = _dev(res.trace, torch.uint8, "trace")
    p = PreparedRollout()
    p.args, p.ref, p.result = a, C.byref(a), res
    p._keep = (own, opp, weights, uniforms, stream_id_dev)
    p._fn = _lib.lib().iago_rollout
    return p


def rollout(own, opp, weights=None, seed=0, id_base=0, stream_id=0, uniforms=None,
            want_final=False, want_turns=False, want_trace=False, out=None,
            throughput_hint=False, stream_id_dev=None):
    """Simulate(state)(color) for every board (mcts_self_play.py:9-134).

    weights=None plays uniformly random legal moves.  `uniforms`
    (IAGO_MAX_TURNS, n) float32 replaces the Philox stream (parity tests).
    `out` may be a RolloutResult with preallocated tensors to reuse.
    throughput_hint: the caller overlaps this launch with others (see
    iago_rollout_args.throughput_hint).
    """
    p = rollout_prepare(own, opp, weights, seed, id_base, stream_id, uniforms, want_final,
                        want_turns, want_trace, out, throughput_hint, stream_id_dev)
    check(p.launch(), "iago_rollout")
    return p.result


ENDGAME_MODES = {"exact": _lib.ENDGAME_EXACT, "wld": _lib.ENDGAME_WLD}
ENDGAME_MOVES = {"best": _lib.ENDGAME_MOVES_BEST, "all": _lib.ENDGAME_MOVES_ALL}
ENDGAME_TIME_LIMIT_MS = 60000

# What a lane search that did not finish everything says, per family: the stack overflow of an unsplit and of a split
# launch, the give-up, the refusals.  limit: the solver's max_empties, the yardstick's depth.
_SOLVER_TEXTS = dict(
    overflow="a position needed more stack frames than max_empties = %(limit)d sizes (ctl[3] set): it was dropped "
             "with solved = 0 and its outputs unwritten",
    job_overflow="a job needed more stack frames than max_empties = %(limit)d sizes (ctl[3] set): it was dropped and its "
                 "root keeps solved = 0",
    gave_up="gave up at its clock limit (%(ms)d ms): %(left)d of %(n)d positions unsolved",
    refused="%(refused)d positions refused (own & opp != 0, or more than max_empties = %(limit)d empties)")
_ALPHABETA_TEXTS = dict(
    overflow="a position needed more stack frames than depth = %(limit)d sizes (ctl[3] set)",
    job_overflow="a job needed more stack frames than depth = %(limit)d sizes (ctl[3] set)",
    gave_up="gave up at its clock limit (%(ms)d ms): %(left)d of %(n)d positions unfinished",
    refused="%(refused)d positions refused (own & opp != 0)")


def alphabeta_job_count(ctl):
    """The jobs a split launch needed, from the host values of its ctl words."""
    return (int(ctl[4]) & 0xFFFFFFFF) | ((int(ctl[5]) & 0xFFFFFFFF) << 32)


def _check_lane_ctl(who, out, ctl, texts, limit, time_limit_ms, n, done_name, job_capacity=None):
    """Raise IagoError (the result `out` as its `result` attribute) unless a lane-search launch finished every position.
    ctl: its words on the host; nothing else is read but, after a give-up, the done flags out[done_name] of its n
    positions.  texts, limit: the family's phrases above.  job_capacity: of a split launch (None: an unsplit one) --
    where the jobs did not fit (ctl[6]) that comes first, with the count needed as the error's `jobs_needed`."""
    gave_up, _, refused, overflow = (int(v) for v in ctl[:4])
    split = job_capacity is not None
    short = split and int(ctl[6]) != 0
    if not (short or gave_up or refused or overflow):
        return
    if short:
        what = "the search needs %d jobs, job_capacity holds %d: nothing was searched" % (
            alphabeta_job_count(ctl), job_capacity)
    elif overflow:
        what = texts["job_overflow" if split else "overflow"] % dict(limit=limit)
    elif gave_up:
        what = texts["gave_up"] % dict(ms=time_limit_ms, left=n - int(out[done_name].sum().item()), n=n)
    else:
        what = texts["refused"] % dict(refused=refused, limit=limit)
    err = _lib.IagoError("%s: %s" % (who, what))
    err.result = out
    if short:
        err.jobs_needed = alphabeta_job_count(ctl)
    raise err


def _check_endgame_ctl(out, n, max_empties, time_limit_ms, who="iago_solve_endgame"):
    """_check_lane_ctl for the solver's entry points, on the ctl words of out (read back here)."""
    _check_lane_ctl(who, out, out["ctl"].tolist(), _SOLVER_TEXTS, max_empties, time_limit_ms, n, "solved")


def endgame_split_arg(split):
    """split of solve_endgame / solve_endgame_moves: 0 (no split), 1 or 2, returned as an int."""
    if isinstance(split, bool) or not isinstance(split, numbers.Integral) or not 0 <= split <= _lib.ENDGAME_MAX_SPLIT:
        raise ValueError("endgame split must be 0, 1 or 2, not %r" % (split,))
    return int(split)


def _job_capacity_arg(job_capacity):
    if job_capacity is not None and (isinstance(job_capacity, bool) or not isinstance(job_capacity, numbers.Integral)
                                     or not 0 <= job_capacity < 2 ** 31):
        raise ValueError("job_capacity must be None or an int in [0, 2^31), not %r" % (job_capacity,))


def _lane_outputs(a, own, opp, score_dtype, done_name, ctl_words, time_limit_ms, best=False, move_score=False):
    """The output dict of a lane-search launch on the positions own / opp -- score, move, nodes, the done flag under its
    name, ctl and, where asked for, best and move_score -- and the inputs that every Args mirror of the family names
    alike, filled in a: the positions, n and time_limit_ms.  The outputs' pointers are _fill_outputs'."""
    n, dev = own.numel(), own.device
    if opp.numel() != n:
        raise ValueError("own/opp sizes differ")
    a.own, a.opp, a.n = _dev(own, torch.int64, "own"), _dev(opp, torch.int64, "opp"), n
    a.time_limit_ms = int(time_limit_ms)
    out = {"score": torch.empty(n, dtype=score_dtype, device=dev), "move": torch.empty(n, dtype=torch.int8, device=dev),
           "nodes": torch.empty(n, dtype=torch.int64, device=dev), done_name: torch.empty(n, dtype=torch.uint8, device=dev),
           "ctl": torch.empty(ctl_words, dtype=torch.int32, device=dev)}
    if best:
        out["best"] = torch.empty(n, dtype=torch.int64, device=dev)
    if move_score:
        out["move_score"] = torch.empty((n, 64), dtype=torch.int8, device=dev)
    return out


def _fill_outputs(a, out, keys=None):
    """a.<key> = the tensor out[key], for the keys named (None: all of out; every Args mirror names them as out does)."""
    for k in out if keys is None else keys:
        setattr(a, k, _dev(out[k], out[k].dtype, k))


def _run_lanes(name, a, out, check_result):
    """The launch of the unsplit entry point `name` on its arguments a; check_result: None, or the check of the host ctl
    words, as _run_split calls it."""
    _fill_outputs(a, out)
    check(getattr(_lib.lib(), name)(C.byref(a), _stream()), name)
    if check_result:
        check_result(out["ctl"].tolist(), None)
    return out


def _run_split(name, a, out, job_capacity, check_result):
    """The launches of the split entry point `name` on its arguments a, which hold everything but the jobs, and the jobs'
    arrays into out.  job_capacity None: the count-only form and one readback first, the arrays then hold the jobs
    exactly.  check_result: None, or what checks the launch -- called with its ctl words on the host and the job
    capacity (a pure function of them: _check_lane_ctl)."""
    entry = getattr(_lib.lib(), name)
    n, dev = int(a.n), out["ctl"].device
    out.update(job_count=torch.empty(n, dtype=torch.int32, device=dev),
               job_first=torch.empty(n, dtype=torch.int64, device=dev))
    _fill_outputs(a, out, ("ctl", "job_count", "job_first"))
    if job_capacity is None:
        # (the count-only form: the job arrays null, and the roots' outputs, which it does not write, too)
        check(entry(C.byref(a), _stream()), name)
        job_capacity = alphabeta_job_count(out["ctl"].tolist())
    _fill_outputs(a, out)
    cap = a.job_capacity = int(job_capacity)
    for k, dt, cols in (("job_own", torch.int64, 1), ("job_opp", torch.int64, 1), ("job_root", torch.int32, 1),
                        ("job_path", torch.int8, 4), ("job_score", out["score"].dtype, 1), ("job_move", torch.int8, 1),
                        ("job_nodes", torch.int64, 1), ("job_done", torch.uint8, 1)):
        # (an empty tensor has no address, and null arrays are the count-only form: room for one job at least)
        t = torch.empty(max(cap, 1) * cols, dtype=dt, device=dev)
        setattr(a, k, _dev(t, dt, k))
        out[k] = t[:cap * cols].reshape(cap, 4) if cols == 4 else t[:cap]
    out["job_capacity"] = cap
    check(entry(C.byref(a), _stream()), name)
    if check_result:
        ctl = out["ctl"].tolist()
        out["jobs"] = alphabeta_job_count(ctl)
        check_result(ctl, cap)
    return out


_SCORE_ONLY = object()   # `moves` of solve_endgame below


def _solve_endgame(own, opp, mode, moves, max_empties, time_limit_ms, check_result, split, job_capacity):
    """solve_endgame (moves: _SCORE_ONLY) and solve_endgame_moves: iago_solve_endgame, iago_solve_endgame_moves or,
    with split > 0, iago_solve_endgame_split."""
    if mode not in ENDGAME_MODES:
        raise ValueError("mode must be 'exact' or 'wld', got %r" % (mode,))
    if moves is not _SCORE_ONLY and moves not in ENDGAME_MOVES:
        raise ValueError("moves must be 'best' or 'all', got %r" % (moves,))
    split = endgame_split_arg(split)
    _job_capacity_arg(job_capacity)
    if split:
        name, a = "iago_solve_endgame_split", _lib.EndgameSplitArgs()
        a.split = split
    elif moves is _SCORE_ONLY:
        name, a = "iago_solve_endgame", _lib.EndgameArgs()
    else:
        name, a = "iago_solve_endgame_moves", _lib.EndgameMovesArgs()
        a.moves = ENDGAME_MOVES[moves]
    a.mode, a.max_empties = ENDGAME_MODES[mode], int(max_empties)
    out = _lane_outputs(a, own, opp, torch.int8, "solved", _lib.ENDGAME_SPLIT_CTL_WORDS if split else _lib.ENDGAME_CTL_WORDS,
                        time_limit_ms, best=moves is not _SCORE_ONLY, move_score=moves == "all")
    checked = check_result and (lambda ctl, cap: _check_lane_ctl(name, out, ctl, _SOLVER_TEXTS, max_empties,
                                                                 time_limit_ms, own.numel(), "solved", cap))
    return _run_split(name, a, out, job_capacity, checked) if split else _run_lanes(name, a, out, checked)


def solve_endgame(own, opp, mode="exact", max_empties=_lib.ENDGAME_MAX_EMPTIES, time_limit_ms=ENDGAME_TIME_LIMIT_MS,
                  check_result=True, split=0, job_capacity=None):
    """The exact value of every position under perfect play (iago_solve_endgame, include/iago_hip_serving.h).

    own / opp: (n,) int64 CUDA tensors, own = side to move.  mode "exact": score = the final disc difference
    #own - #opp (empty squares count for nobody); "wld": its sign only (much cheaper).  Returns a dict of device
    tensors: score (n,) int8, move (n,) int8 = the lowest-indexed move reaching the score (-1: the side to move must
    pass, -2: the game is over), nodes (n,) int64, solved (n,) uint8, ctl (4,) int32.
    check_result (one host sync): raise IagoError when the launch gave up at time_limit_ms, refused a position
    (own & opp != 0, more than max_empties empties) or dropped one for want of stack (ctl[3]); the result is the
    error's `result` attribute.

    split = 1 or 2 (0, the default: the call above, argument for argument; anything else is a ValueError): the same
    score, move and solved from iago_solve_endgame_split, which spreads every root's search over the lanes -- the first
    `split` plies expanded into jobs on the device, the jobs solved a lane each with the full window, their values taken
    back per root.  nodes is then the nodes expanded + the jobs' own.  job_capacity: the jobs the launch has room for;
    None takes a count-only launch and one readback first and allocates exactly, an int takes no readback -- where the
    jobs do not fit nothing is searched, every solved is 0, ctl[6] is set, and check_result raises an IagoError with the
    count needed in `jobs_needed`.  The dict then also holds ctl (8,) int32 (ctl[4] / [5]: the jobs needed), job_count
    (n,) int32, job_first (n,) int64, the job arrays job_own, job_opp, job_root, job_path (the job's empties, first
    move, second move, 0), job_score, job_move, job_nodes, job_done, job_capacity and, with check_result, `jobs`."""
    return _solve_endgame(own, opp, mode, _SCORE_ONLY, max_empties, time_limit_ms, check_result, split, job_capacity)


def solve_endgame_moves(own, opp, mode="exact", moves="best", max_empties=_lib.ENDGAME_MAX_EMPTIES,
                        time_limit_ms=ENDGAME_TIME_LIMIT_MS, check_result=True, split=0, job_capacity=None):
    """solve_endgame with EVERY optimal move (iago_solve_endgame_moves, include/iago_hip_serving.h).

    Returns solve_endgame's dict (score and move are its own, bit for bit) plus best (n,) int64: bit a set iff move a
    reaches the score (0: the mover must pass, the game is over, the position was refused).  moves "best": the set
    alone (about 1.1 x solve_endgame's nodes); "all": every legal move is searched with the full window, and
    move_score (n, 64) int8 holds the value of move a from the mover's view, -128 (IAGO_ENDGAME_NO_MOVE) on every cell
    that is no legal move of the mover (about 2.2 x the nodes).  check_result: as in solve_endgame.
    split = 1 or 2, job_capacity: as in solve_endgame -- the same best and move_score from iago_solve_endgame_split,
    whose jobs know every root move's exact value under either `moves`; the dict also holds its job arrays."""
    return _solve_endgame(own, opp, mode, moves, max_empties, time_limit_ms, check_result, split, job_capacity)


def play_endgame(own, opp, turn, stones, pass_flg, parked=None, max_turns=IAGO_MAX_TURNS,
                 max_empties=_lib.ENDGAME_MAX_EMPTIES, time_limit_ms=ENDGAME_TIME_LIMIT_MS, records=None,
                 check_result=True, best=False):
    """The parked games of a batch to their end under perfect play (iago_play_endgame, include/iago_hip_serving.h):
    both sides play iago_solve_endgame's EXACT move at every turn, with the books of the whole-game search.

    own / opp (n,) int64, own = the side to move; turn / stones (n,) int32; pass_flg (n,) uint8; parked (n,) uint8,
    None = every game.  own, opp and turn are UPDATED IN PLACE for the games played: the final position (own = the side
    that would move next) and the turns the game took.  records: None (fresh zeroed tensors, move -1), or a dict of
    (max_turns, stride) tensors own, opp (int64), valid (uint8), move, score (int8) whose rows from each game's turn on
    are written.  Returns the dict of the records + finished (n,) uint8 and ctl (4,) int32.  check_result (one host
    sync): raise IagoError unless every parked game was played to its end (the clock limit, a game refused for
    own & opp != 0, more than max_empties empties or a turn outside the records; the result is the error's `result`).
    best=True (iago_play_endgame_moves): one more record, best (max_turns, stride) int64 -- the set of the moves reaching
    the turn's score on every solved turn, 0 where valid is 0; records, when given, then holds it too.  Everything else
    is the same, bit for bit."""
    n = own.numel()
    dev = own.device
    for name, t in (("opp", opp), ("turn", turn), ("stones", stones), ("pass_flg", pass_flg)):
        if t.numel() != n:
            raise ValueError("own / %s sizes differ" % name)
    if parked is None:
        parked = torch.ones(n, dtype=torch.uint8, device=dev)
    elif parked.numel() != n:
        raise ValueError("own / parked sizes differ")
    T = int(max_turns)
    if records is None:
        records = dict(own=torch.zeros((T, n), dtype=torch.int64, device=dev),
                       opp=torch.zeros((T, n), dtype=torch.int64, device=dev),
                       valid=torch.zeros((T, n), dtype=torch.uint8, device=dev),
                       move=torch.full((T, n), -1, dtype=torch.int8, device=dev),
                       score=torch.zeros((T, n), dtype=torch.int8, device=dev))
        if best:
            records["best"] = torch.zeros((T, n), dtype=torch.int64, device=dev)
    stride = records["own"].shape[1] if records["own"].dim() == 2 else n
    for k in ("own", "opp", "valid", "move", "score") + (("best",) if best else ()):
        if tuple(records[k].shape) != (T, stride):
            raise ValueError("records[%r] must be (max_turns, stride) = (%d, %d)" % (k, T, stride))
    out = dict(records)
    out["finished"] = torch.empty(n, dtype=torch.uint8, device=dev)
    out["ctl"] = torch.empty(_lib.ENDGAME_CTL_WORDS, dtype=torch.int32, device=dev)
    m = _lib.PlayEndgameMovesArgs()
    a = m.play if best else _lib.PlayEndgameArgs()
    a.own, a.opp, a.turn = _dev(own, torch.int64, "own"), _dev(opp, torch.int64, "opp"), _dev(turn, torch.int32, "turn")
    a.stones, a.pass_flg = _dev(stones, torch.int32, "stones"), _dev(pass_flg, torch.uint8, "pass_flg")
    a.parked, a.n, a.stride = _dev(parked, torch.uint8, "parked"), n, stride
    a.max_turns, a.max_empties, a.time_limit_ms = T, int(max_empties), int(time_limit_ms)
    a.rec_own, a.rec_opp = _dev(out["own"], torch.int64, "records own"), _dev(out["opp"], torch.int64, "records opp")
    a.rec_valid, a.rec_move = _dev(out["valid"], torch.uint8, "records valid"), _dev(out["move"], torch.int8, "records move")
    a.rec_score = _dev(out["score"], torch.int8, "records score")
    a.finished, a.ctl = _dev(out["finished"], torch.uint8, "finished"), _dev(out["ctl"], torch.int32, "ctl")
    if best:
        m.rec_best = _dev(out["best"], torch.int64, "records best")
        check(_lib.lib().iago_play_endgame_moves(C.byref(m), _stream()), "iago_play_endgame_moves")
    else:
        check(_lib.lib().iago_play_endgame(C.byref(a), _stream()), "iago_play_endgame")
    if check_result:
        back = torch.cat([out["ctl"].to(torch.int64), (out["finished"] != parked).sum().reshape(1)]).tolist()
        check_play_endgame(back, out, max_empties, time_limit_ms)
    return out


def check_play_endgame(back, out, max_empties, time_limit_ms):
    """Raise IagoError unless iago_play_endgame played every parked game to its end; back: its four ctl words and the
    number of games with finished != parked, read back by the caller."""
    gave_up, _, refused, overflow, unfinished = (int(v) for v in back)
    if not (gave_up or refused or overflow or unfinished):
        return
    if gave_up:
        what = "gave up at its clock limit (%d ms)" % time_limit_ms
    elif refused:
        what = ("%d games refused (own & opp != 0, more than max_empties = %d empties, or a turn outside the records)"
                % (refused, max_empties))
    else:
        what = "a game needed more stack frames than max_empties = %d sizes (ctl[3] set)" % max_empties
    err = _lib.IagoError("iago_play_endgame: %s: %d games not played to their end" % (what, unfinished))
    err.result = out
    raise err


def alphabeta_depth_arg(depth):
    """depth of alphabeta_moves / engine.AlphaBeta: an int in [1, 10], returned as an int."""
    if isinstance(depth, bool) or not isinstance(depth, numbers.Integral) or not 1 <= depth <= _lib.ALPHABETA_MAX_DEPTH:
        raise ValueError("alpha-beta depth must be an int in [1, %d], not %r" % (_lib.ALPHABETA_MAX_DEPTH, depth))
    return int(depth)


def alphabeta_split_arg(split, depth):
    """split of alphabeta_moves / engine.AlphaBeta beside its depth: 0 (no split), 1 or 2, and below depth; returned as
    an int."""
    if isinstance(split, bool) or not isinstance(split, numbers.Integral) or not 0 <= split <= _lib.ALPHABETA_MAX_SPLIT:
        raise ValueError("alpha-beta split must be 0, 1 or 2, not %r" % (split,))
    if split >= depth:
        raise ValueError("alpha-beta split must be below the depth: split %d at depth %d" % (split, depth))
    return int(split)


def alphabeta_moves(own, opp, depth, time_limit_ms=ENDGAME_TIME_LIMIT_MS, check_result=True, split=0, job_capacity=None):
    """A fixed-depth alpha-beta search on a hand-written evaluation for every position (iago_alphabeta_moves,
    include/iago_hip_serving.h): the opponent that owes nothing to the nets.

    own / opp: (n,) int64 CUDA tensors, own = side to move; depth: an int in [1, 10] (ValueError otherwise), one value
    per launch.  Returns a dict of device tensors: score (n,) int16 = search(own, opp, depth), move (n,) int8 = the
    lowest-indexed move whose value equals the score (-1: the side to move must pass, -2: the game is over), nodes
    (n,) int64, done (n,) uint8, ctl (4,) int32.  check_result (one host sync): raise IagoError when the launch gave up
    at time_limit_ms, refused a position (own & opp != 0) or overflowed its stack (ctl[3]); the result is the error's
    `result` attribute.

    split = 1 or 2 (0, the default: the call above, argument for argument; anything else, or split >= depth, is a
    ValueError): the same score, move and done from iago_alphabeta_moves_split, which spreads every root's search over
    the lanes -- the first `split` plies expanded into jobs on the device, the jobs searched a lane each, their values
    taken back per root.  nodes is then the nodes expanded + the jobs' own.  job_capacity: the jobs the launch has room
    for; None takes a count-only launch and one readback first and allocates exactly, an int takes no readback -- where
    the jobs do not fit nothing is searched, every done is 0, ctl[6] is set, and check_result raises an IagoError with
    the count needed in `jobs_needed`.  The dict then also holds ctl (8,) int32 (ctl[4] / [5]: the jobs needed),
    job_count (n,) int32, job_first (n,) int64, the job arrays job_own, job_opp, job_root, job_path (depth left, first
    move, second move, 0), job_score, job_move, job_nodes, job_done, job_capacity and, with check_result, `jobs`."""
    depth = alphabeta_depth_arg(depth)
    split = alphabeta_split_arg(split, depth)
    _job_capacity_arg(job_capacity)
    if split:
        name, a = "iago_alphabeta_moves_split", _lib.AlphaBetaSplitArgs()
        a.split = split
    else:
        name, a = "iago_alphabeta_moves", _lib.AlphaBetaArgs()
    a.depth = depth
    out = _lane_outputs(a, own, opp, torch.int16, "done", _lib.ALPHABETA_SPLIT_CTL_WORDS if split else _lib.ENDGAME_CTL_WORDS,
                        time_limit_ms)
    checked = check_result and (lambda ctl, cap: _check_lane_ctl(name, out, ctl, _ALPHABETA_TEXTS, depth, time_limit_ms,
                                                                 own.numel(), "done", cap))
    return _run_split(name, a, out, job_capacity, checked) if split else _run_lanes(name, a, out, checked)


def random_moves(own, opp, seed, id_base, id_mod, turn):
    """The random opening draw (iago_random_moves, include/iago_hip_serving.h): (n,) int8, the move of every game's mover
    (own to move) -- with K >= 1 legal moves the r-th lowest legal cell, r = (w * K) >> 32, w = word turn & 3 of
    Philox4x32-10 on (id_base + g mod id_mod, turn >> 2, 0, 0) under seed ^ OPENING_SEED_XOR; -1 where it has none."""
    n = own.numel()
    if opp.numel() != n:
        raise ValueError("own/opp sizes differ")
    move = torch.empty(n, dtype=torch.int8, device=own.device)
    check(_lib.lib().iago_random_moves(_dev(own, torch.int64, "own"), _dev(opp, torch.int64, "opp"), n,
                                       C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), int(id_base) & 0xFFFFFFFF, int(id_mod),
                                       int(turn), _dev(move, torch.int8, "move"), _stream()), "iago_random_moves")
    return move


def explore_turns_arg(k):
    """explore_turns of SelfPlayEngine.play / play_stream: None or 0 (off: None is returned), or a positive int (at most
    IAGO_MAX_TURNS turns are drawn, a larger value means every turn)."""
    if k is None:
        return None
    if isinstance(k, bool) or not isinstance(k, numbers.Integral) or k < 0:
        raise ValueError("explore_turns must be None or an int >= 0, not %r" % (k,))
    return min(int(k), IAGO_MAX_TURNS) or None


def draw_move(tree, active, seed, game_id, turn, move, visits=None):
    """iago_mcts_draw_move (include/iago_hip_serving.h): iago_mcts_best_move's sibling for exploring self-play.  move[g]
    (int8) of every game with active[g] != 0 (active None: every game) is drawn in proportion to the visit counts of the
    children of its tree's root: N = their sum, w = word turn[g] & 3 of Philox4x32-10 on (game_id[g], turn[g] >> 2, 0, 0)
    under seed ^ EXPLORE_SEED_XOR, r = (w * N) >> 32, the lowest cell a with sum_{b <= a} n[b] > r (N == 0: the first
    maximum; no children: -2).  tree: a pointer to the iago_mcts_tree (TreePool.ref()); game_id / turn (n_games,) int32,
    game_id the GLOBAL ids (id_base + g) as their 32 bits; visits: optional (n_games, 64) int32, the visit row."""
    check(_lib.lib().iago_mcts_draw_move(tree, _dev(active, torch.uint8, "active") if active is not None else None,
                                         C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), _dev(game_id, torch.int32, "game_id"),
                                         _dev(turn, torch.int32, "turn"), _dev(move, torch.int8, "move"),
                                         _dev(visits, torch.int32, "visits") if visits is not None else None, _stream()),
          "iago_mcts_draw_move")
    return move, visits


def search_explore(args, explore_turns, streams=None, park=None):
    """iago_mcts_search_explore (include/iago_hip_serving.h): the whole-game launch of `args` (a _lib.MctsSearchArgs)
    whose searched moves of the turns below explore_turns are drawn from the visit counts; streams: the role split's
    handle or None; park: a _lib.SearchParkArgs (the hand-over of iago_mcts_search_park in the same launch) or None.
    The caller keeps `args`, `park` and everything they point to alive until the launch has run."""
    e = _lib.SearchExploreArgs()
    e.explore_turns = int(explore_turns)
    e.streams = streams
    e.park = C.addressof(park) if park is not None else None
    check(_lib.lib().iago_mcts_search_explore(C.byref(args), C.byref(e), _stream()), "iago_mcts_search_explore")


def playout_cap_arg(cap, n_sims):
    """playout_cap of SelfPlayEngine.play / play_stream: None (off), or (n_fast, full_per_256) -- two ints, 1 <= n_fast <=
    n_sims and 1 <= full_per_256 <= 256 -- returned as a tuple of ints."""
    if cap is None:
        return None
    try:
        n_fast, full = cap
    except (TypeError, ValueError):
        raise ValueError("playout_cap must be None or (n_fast, full_per_256), not %r" % (cap,))
    for v in (n_fast, full):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise ValueError("playout_cap must be None or (n_fast, full_per_256), two ints, not %r" % (cap,))
    if not 1 <= n_fast <= int(n_sims):
        raise ValueError("playout_cap: n_fast must be in [1, n_sims = %d], not %r" % (int(n_sims), n_fast))
    if not 1 <= full <= 256:
        raise ValueError("playout_cap: full_per_256 must be in [1, 256], not %r" % (full,))
    return int(n_fast), int(full)


def playout_cap_mask(seed, game_id, turn, full_per_256, out=None):
    """iago_mcts_cap_mask (include/iago_hip_serving.h): (n,) uint8, 1 where turn[i] of the game with GLOBAL id game_id[i]
    (id_base + g, as its 32 bits) is a FAST turn of the playout cap: word turn & 3 of Philox4x32-10 on (game_id, turn >> 2,
    0, 0) under seed ^ CAP_SEED_XOR, fast iff (w >> 24) >= full_per_256.  game_id / turn: (n,) int32."""
    n = game_id.numel()
    if out is None:
        out = torch.empty(n, dtype=torch.uint8, device=game_id.device)
    check(_lib.lib().iago_mcts_cap_mask(C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), _dev(game_id, torch.int32, "game_id"),
                                        _dev(turn, torch.int32, "turn"), int(full_per_256), n, _dev(out, torch.uint8, "fast"),
                                        _stream()), "iago_mcts_cap_mask")
    return out


def search_cap(args, n_fast, full_per_256, explore_turns=0, streams=None, park=None):
    """iago_mcts_search_cap (include/iago_hip_serving.h): the whole-game launch of `args` (a _lib.MctsSearchArgs) under
    playout-cap randomisation -- a searched turn is full (args.n_sims playouts, valid 1) with probability full_per_256 /
    256, else fast (n_fast playouts, valid 4); explore_turns, streams, park: as search_explore takes them.  The caller
    keeps `args`, `park` and everything they point to alive until the launch has run."""
    c = _lib.SearchCapArgs()
    c.n_fast, c.full_per_256, c.explore_turns = int(n_fast), int(full_per_256), int(explore_turns or 0)
    c.streams = streams
    c.park = C.addressof(park) if park is not None else None
    check(_lib.lib().iago_mcts_search_cap(C.byref(args), C.byref(c), _stream()), "iago_mcts_search_cap")


def root_noise_arg(noise):
    """root_noise of SelfPlayEngine.play / play_stream / BatchedMCTS.search: None (off), or (alpha_256, eps_256[, draws])
    -- ints, 1 <= alpha_256 <= 4096 (alpha = alpha_256 / 256), 0 <= eps_256 <= 256 (eps = eps_256 / 256), draws a power of
    two in [16, 1024] (default _lib.NOISE_DRAWS) -- returned as a tuple of three ints."""
    if noise is None:
        return None
    what = "root_noise must be None or (alpha_256, eps_256[, draws]), ints, not %r" % (noise,)
    try:
        vals = tuple(noise)
    except TypeError:
        raise ValueError(what)
    if len(vals) not in (2, 3) or any(isinstance(v, bool) or not isinstance(v, numbers.Integral) for v in vals):
        raise ValueError(what)
    alpha, eps, draws = (vals + (_lib.NOISE_DRAWS,))[:3]
    if not 1 <= alpha <= 4096:
        raise ValueError("root_noise: alpha_256 must be in [1, 4096], not %r" % (alpha,))
    if not 0 <= eps <= 256:
        raise ValueError("root_noise: eps_256 must be in [0, 256], not %r" % (eps,))
    if not 16 <= draws <= 1024 or draws & (draws - 1):
        raise ValueError("root_noise: draws must be a power of two in [16, 1024], not %r" % (draws,))
    return int(alpha), int(eps), int(draws)


def _root_noise_struct(noise, counts, into=None):
    nz = _lib.RootNoise() if into is None else into
    nz.alpha_256, nz.eps_256, nz.draws = (int(v) for v in noise)
    # (the counts, 0 .. 1024, as int16: the same bits as the library's uint16, and a dtype every torch op takes)
    nz.counts = _dev(counts, torch.int16, "counts") if counts is not None else None
    return nz


def root_noise(tree, active, root_own, root_opp, seed, game_id, turn, noise, counts):
    """iago_mcts_root_noise (include/iago_hip_serving.h): the root noise of the turn loop.  For every game with active[g]
    != 0 (active None: every game) the Polya urn of turn[g] of the game with GLOBAL id game_id[g] over the legal moves of
    the mover of (root_own[g], root_opp[g]) -- noise = (alpha_256, eps_256, draws); draw j takes the lowest legal cell a
    with sum_{b <= a} (alpha_256 + 256 c[b]) > (w_j * (K alpha_256 + 256 j)) >> 32, w_j word j & 3 of Philox4x32-10 on
    (game_id, turn, j >> 2, 0) under seed ^ NOISE_SEED_XOR -- written to counts[g] ((n_games, 64) int16, 0 off the legal
    set and for K < 2), and the mix p * (256 - eps_256) / 256 + eps_256 c / (256 draws) applied to the children the tree's
    root already has.  Inactive games' rows and trees are not touched.  tree: TreePool.ref(); game_id / turn (n_games,)
    int32.  Returns counts."""
    nz = _root_noise_struct(noise, counts)
    check(_lib.lib().iago_mcts_root_noise(tree, _dev(active, torch.uint8, "active") if active is not None else None,
                                          _dev(root_own, torch.int64, "root_own"), _dev(root_opp, torch.int64, "root_opp"),
                                          C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), _dev(game_id, torch.int32, "game_id"),
                                          _dev(turn, torch.int32, "turn"), C.byref(nz), _stream()), "iago_mcts_root_noise")
    return counts


def search_noise(args, noise, counts, streams=None):
    """iago_mcts_search_noise (include/iago_hip_serving.h): the ONE search of `args` (a _lib.MctsSearchArgs, max_turns 0)
    in which a root that expands creates its children with the mixed priors of its row of `counts` -- the (n_games, 64)
    int16 rows root_noise() left for this turn; noise = (alpha_256, eps_256, draws) as given there; streams: the role
    split's handle or None.  The caller keeps `args`, `counts` and everything they point to alive until the launch has
    run."""
    z = _lib.SearchNoiseArgs()
    _root_noise_struct(noise, counts, z.noise)
    z.streams = streams
    check(_lib.lib().iago_mcts_search_noise(C.byref(args), C.byref(z), _stream()), "iago_mcts_search_noise")


def forced_playouts_arg(k_256, noise):
    """forced_playouts of SelfPlayEngine.play / play_stream / BatchedMCTS.search: None (off), or k_256, an int in [1,
    4096] (k = k_256 / 256; KataGo's k = 2 is 512), which requires root noise (`noise` as root_noise_arg returned it;
    root_noise=(alpha_256, 0) forces without mixing).  Returned as an int."""
    if k_256 is None:
        return None
    if isinstance(k_256, bool) or not isinstance(k_256, numbers.Integral) or not 1 <= k_256 <= 4096:
        raise ValueError("forced_playouts must be None or an int k_256 in [1, 4096], not %r" % (k_256,))
    if noise is None:
        raise ValueError("forced_playouts requires root_noise (root_noise=(alpha_256, 0) forces without mixing)")
    return int(k_256)


def search_forced(args, noise, counts, k_256, streams=None):
    """iago_mcts_search_forced (include/iago_hip_serving.h): search_noise() with forced playouts -- at the ROOT of every
    active game's search, when it has two or more children, a child with n >= 1 visits and stored prior p for which
    float64(256 n n) < (float64(k_256) * float64(p)) * float64(N), N the root's visits, scores +inf in Node.select.
    args, noise, counts, streams: as search_noise takes them; k_256 an int in [1, 4096]."""
    z = _lib.SearchForcedArgs()
    _root_noise_struct(noise, counts, z.noise)
    z.streams = streams
    z.k_256 = int(k_256)
    check(_lib.lib().iago_mcts_search_forced(C.byref(args), C.byref(z), _stream()), "iago_mcts_search_forced")


def prune_visits(tree, active, c_puct, k_256, pruned, flags=0):
    """iago_mcts_prune_visits (include/iago_hip_serving.h): the policy-target pruning of forced playouts.  For every game
    with active[g] != 0 (active None: every game) the visit row of the tree's root into pruned[g] ((n_games, 64) int32)
    with, for a root of K >= 2 children, every child c other than the first most visited one b reduced from its n visits
    to m: F = the number of j in 1 .. n - 1 with forced(j, p_c, N); m = n; while n - m < F and the PUCT score of c with
    m - 1 visits is below b's score, m -= 1; m = 0 if m < n and m == 1.  Fewer than two children: the raw row.  Inactive
    games' rows are not touched; the trees are only read.  tree: TreePool.ref().  Returns pruned.
    flags: 0, or _lib.SEARCH_PUCT_AZ for the trees of a search under the AlphaZero selection rule -- the scores then have
    its denominator (iago_mcts_prune_visits_rule)."""
    if flags:
        check(_lib.lib().iago_mcts_prune_visits_rule(tree, _dev(active, torch.uint8, "active") if active is not None else None,
                                                     C.c_float(float(c_puct)), int(k_256), int(flags),
                                                     _dev(pruned, torch.int32, "pruned"), _stream()),
              "iago_mcts_prune_visits_rule")
        return pruned
    check(_lib.lib().iago_mcts_prune_visits(tree, _dev(active, torch.uint8, "active") if active is not None else None,
                                            C.c_float(float(c_puct)), int(k_256), _dev(pruned, torch.int32, "pruned"),
                                            _stream()), "iago_mcts_prune_visits")
    return pruned


def gumbel_arg(gumbel):
    """gumbel of SelfPlayEngine.play / play_stream / play_match / BatchedMCTS.search / MCTS: None (off), or (m,
    c_scale_256[, c_visit]) -- ints, 2 <= m <= 64 (the moves considered), 1 <= c_scale_256 <= 4096 (c_scale =
    c_scale_256 / 256), 0 <= c_visit <= 4096 (default _lib.GUMBEL_C_VISIT) -- returned as a tuple of three ints."""
    if gumbel is None:
        return None
    what = "gumbel must be None or (m, c_scale_256[, c_visit]), ints, not %r" % (gumbel,)
    try:
        vals = tuple(gumbel)
    except TypeError:
        raise ValueError(what)
    if len(vals) not in (2, 3) or any(isinstance(v, bool) or not isinstance(v, numbers.Integral) for v in vals):
        raise ValueError(what)
    m, c_scale, c_visit = (vals + (_lib.GUMBEL_C_VISIT,))[:3]
    if not 2 <= m <= 64:
        raise ValueError("gumbel: m must be in [2, 64], not %r" % (m,))
    if not 1 <= c_scale <= 4096:
        raise ValueError("gumbel: c_scale_256 must be in [1, 4096], not %r" % (c_scale,))
    if not 0 <= c_visit <= 4096:
        raise ValueError("gumbel: c_visit must be in [0, 4096], not %r" % (c_visit,))
    return int(m), int(c_scale), int(c_visit)


_GUMBEL_TABLES = []


def gumbel_tables():
    """The two tables of the Gumbel root search (include/iago_hip_serving.h), computed once in numpy float64 and read as
    they are by the device and by tests/gumbel_ref.py: (gumbel_q16, ln_q16), int32 arrays of 65536 and 4096 entries --
    round(65536 * -ln(-ln((u + 0.5) / 65536))) and round(65536 * ln(1 + (i + 0.5) / 4096)).  Read-only."""
    if not _GUMBEL_TABLES:
        u = (np.arange(65536, dtype=np.float64) + 0.5) / 65536.0
        g = np.rint(65536.0 * -np.log(-np.log(u))).astype(np.int32)
        ln = np.rint(65536.0 * np.log1p((np.arange(4096, dtype=np.float64) + 0.5) / 4096.0)).astype(np.int32)
        g.setflags(write=False)
        ln.setflags(write=False)
        _GUMBEL_TABLES.extend((g, ln))
    return _GUMBEL_TABLES[0], _GUMBEL_TABLES[1]


def gumbel_schedule(m, n_sims):
    """The sequential-halving schedule of the Gumbel root search (include/iago_hip_serving.h): int16 [m + 1][n_sims], row k
    the visit count the next considered move must have, playout by playout, when k moves are considered.  Rows 0 and 1
    count 0, 1, 2, ...; row k >= 2: k counters at 0, L = ceil(log2 k), cur = k, and until the row is full extra = max(1,
    n_sims // (L cur)) times the first cur counters are written and each of them grows by one, then cur = max(2, cur //
    2).  m in [1, 64], n_sims in [1, 32767]."""
    m, n_sims = int(m), int(n_sims)
    if not 1 <= m <= 64 or not 1 <= n_sims <= 32767:
        raise ValueError("gumbel_schedule: m in [1, 64] and n_sims in [1, 32767] expected, not %r, %r" % (m, n_sims))
    out = np.zeros((m + 1, n_sims), np.int16)
    out[0] = out[1] = np.arange(n_sims)
    for k in range(2, m + 1):
        row, counters = [], [0] * k
        levels, cur = (k - 1).bit_length(), k
        while len(row) < n_sims:
            for _ in range(max(1, n_sims // (levels * cur))):
                row.extend(counters[:cur])
                counters[:cur] = [c + 1 for c in counters[:cur]]
                if len(row) >= n_sims:
                    break
            cur = max(2, cur // 2)
        out[k] = row[:n_sims]
    return out


def _gumbel_struct(gumbel, tables, sched, g, into=None):
    """gumbel = (m, c_scale_256, c_visit); tables = (gumbel_q16, ln_q16) on the device; sched (m + 1, n_sims) int16 on the
    device or None (the draw and the finish do not read it); g (n_games, 64) int32."""
    z = _lib.GumbelRoot() if into is None else into
    z.m, z.c_scale_256, z.c_visit = (int(v) for v in gumbel)
    z.gumbel_q16, z.ln_q16 = _dev(tables[0], torch.int32, "gumbel_q16"), _dev(tables[1], torch.int32, "ln_q16")
    z.sched = _dev(sched, torch.int16, "sched") if sched is not None else None
    z.g = _dev(g, torch.int32, "g") if g is not None else None
    return z


def gumbel_draw(tree, active, seed, game_id, turn, gumbel, tables, g):
    """iago_mcts_gumbel_draw (include/iago_hip_serving.h): the Gumbel root search's draw for the turn loop.  For every
    game with active[g] != 0 (active None: every game) and every cell a: g[game][a] = gumbel_q16[c0 >> 16], c0 word 0 of
    Philox4x32-10 on (game_id, turn, a, 0) under seed ^ GUMBEL_SEED_XOR.  Inactive games' rows are not touched.  tree:
    TreePool.ref(); game_id / turn (n_games,) int32; tables: gumbel_tables() on the device; g (n_games, 64) int32.
    Returns g."""
    z = _gumbel_struct(gumbel, tables, None, g)
    check(_lib.lib().iago_mcts_gumbel_draw(tree, _dev(active, torch.uint8, "active") if active is not None else None,
                                           C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), _dev(game_id, torch.int32, "game_id"),
                                           _dev(turn, torch.int32, "turn"), C.byref(z), _stream()), "iago_mcts_gumbel_draw")
    return g


def search_gumbel(args, gumbel, tables, sched, g, streams=None):
    """iago_mcts_search_gumbel (include/iago_hip_serving.h): the ONE search of `args` (a _lib.MctsSearchArgs, max_turns 0,
    negamax backup and AlphaZero selection, fresh roots) with the Gumbel rule at every active game's root -- a child
    whose visits are sched[min(m, K)][min(t, n_sims - 1)] scores g + logit_q16(p) + sigma, every other child -inf.
    sched: gumbel_schedule(m, args.n_sims) on the device; g: the rows gumbel_draw() left for this turn; streams: the
    role split's handle or None.  The caller keeps everything alive until the launch has run."""
    z = _lib.SearchGumbelArgs()
    _gumbel_struct(gumbel, tables, sched, g, z.gumbel)
    z.streams = streams
    check(_lib.lib().iago_mcts_search_gumbel(C.byref(args), C.byref(z), _stream()), "iago_mcts_search_gumbel")


def gumbel_finish(tree, active, gumbel, tables, g, move, n, q, logit):
    """iago_mcts_gumbel_finish (include/iago_hip_serving.h): the move of the Gumbel root search -- of the root's children
    with the most visits the first maximum of g + logit_q16(p) + sigma; one child or none: best_move's answer -- into
    move (n_games,) int8, and the rows n (int32), q (float32, 0 where unvisited) and logit (int32, INT32_MIN off the root's
    children), (n_games, 64) each.  Inactive games are not touched; the trees are only read."""
    z = _gumbel_struct(gumbel, tables, None, g)
    check(_lib.lib().iago_mcts_gumbel_finish(tree, _dev(active, torch.uint8, "active") if active is not None else None,
                                             C.byref(z), _dev(move, torch.int8, "move"), _dev(n, torch.int32, "n"),
                                             _dev(q, torch.float32, "q"), _dev(logit, torch.int32, "logit"), _stream()),
          "iago_mcts_gumbel_finish")
    return move


def search_arena(args_a, args_b, check_result=True):
    """iago_mcts_search_arena (include/iago_hip_serving.h): the searches of `args_a` and `args_b` (two
    _lib.MctsSearchArgs, each a complete search of iago_mcts_search_persistent with its own nets, trees and rings) in
    ONE launch.  Either may be None (the library refuses it, like everything else it documents).  Returns the library's
    code; check_result (default): anything but IAGO_OK raises IagoError -- with the code in its `rc` -- instead.  The
    caller keeps both sets and everything they point to alive until the launch has run."""
    rc = _lib.lib().iago_mcts_search_arena(C.byref(args_a) if args_a is not None else None,
                                           C.byref(args_b) if args_b is not None else None, _stream())
    if check_result and rc != _lib.IAGO_OK:
        try:
            check(rc, "iago_mcts_search_arena")
        except _lib.IagoError as err:
            err.rc = rc
            raise
    return rc
