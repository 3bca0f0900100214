"""What the tests know about the persistent search's request rings (iago_amd/csrc/search_request.hpp: a request's words,
a ring's granules; iago_amd/csrc/search_kernel.hip: send_request, ring_backlog, ring_take, ring_fetch, claim; the
engine's m._ps["ctl"] and m._ps["q_slots"], which a launch zeroes at its start and leaves as they were at its end).

Two rings, one per kind of net work (VALUE = 0, POLICY = 1), of QCAP slots of SLOT_STRIDE uint64 granules.  Ring q has two
uint32 counters in ctl: the tail (ctl[9 + 2q]: entries reserved by send_request, one fetch-and-add per request) and the
head (ctl[8 + 2q]: tickets handed out to net workgroups, one fetch-and-add per ticket).  Ticket t belongs to the entry
in slot_of(t) = t % QCAP.  The entry is WORDS granules, granule i = (t + 1) << 32 | word i of the request:

  [0] who: the kind bit (bit 31, = the ring) | the game (the slot whose mailbox takes the reply), or NOBODY;
  [1] the reply's tag;
  [2] own lo, [3] own hi, [4] opp lo, [5] opp hi: the position, own = the side to move.

A reply is one granule: tag << 32 | the float32's bits."""
import numpy as np

QCAP = 4096                  # IAGO_SEARCH_QUEUE_ENTRIES
SLOT_STRIDE = 8
W_WHO, W_TAG, W_OWN_LO, W_OWN_HI, W_OPP_LO, W_OPP_HI, WORDS = range(7)
NOBODY = 0x7FFFFFFF
KIND_VALUE, KIND_POLICY = 0, 1
CTL_FINISHED, CTL_ABORT, CTL_NET_WGS = 2, 3, 7
LOW = np.uint64(0xFFFFFFFF)
# totals: [0] value requests a game waits for, [1] policy requests, [3] pair walks, [11] value requests of NOBODY
T_VALUE, T_POLICY, T_PAIRS, T_AHEAD = 0, 1, 3, 11


def ctl_head(q):
    return 8 + 2 * q


def ctl_tail(q):
    return 9 + 2 * q


def slot_of(t):
    return int(t) % QCAP


def last_ticket(slot, tail):
    """The last ticket below `tail` that maps to `slot`; None: no ticket reached the slot."""
    if tail <= slot:
        return None
    return slot + (tail - 1 - slot) // QCAP * QCAP


def entry_word(t, x):
    return ((int(t) + 1) & 0xFFFFFFFF) << 32 | int(x)


def who_word(kind, game):
    return int(kind) << 31 | int(game)


def entry(t, kind, game, tag, own, opp):
    """The SLOT_STRIDE granules send_request writes for ticket t (the unused ones: 0)."""
    words = (who_word(kind, game), tag, own & 0xFFFFFFFF, own >> 32, opp & 0xFFFFFFFF, opp >> 32)
    return np.array([entry_word(t, w) for w in words] + [0] * (SLOT_STRIDE - WORDS), dtype=np.uint64)


def decode(e):
    """An entry's granules -> dict(tags: the WORDS high halves, kind, game, tag, own, opp)."""
    e = np.asarray(e, dtype=np.uint64)
    w = [int(x) for x in (e[:WORDS] & LOW)]
    return dict(tags=[int(x) for x in (e[:WORDS] >> np.uint64(32))], kind=w[W_WHO] >> 31, game=w[W_WHO] & 0x7FFFFFFF,
                tag=w[W_TAG], own=w[W_OWN_HI] << 32 | w[W_OWN_LO], opp=w[W_OPP_HI] << 32 | w[W_OPP_LO])


def reply_word(tag, bits):
    return int(tag) << 32 | int(bits)


def reply_tag(x):
    return int(x) >> 32 & 0xFFFFFFFF


def reply_bits(x):
    return int(x) & 0xFFFFFFFF


def read(m):
    """Host copies after m's last launch: (ctl uint32 [16], heads [2], tails [2], entries uint64 [2][QCAP][SLOT_STRIDE])."""
    import torch
    torch.cuda.synchronize()
    ctl = m._ps["ctl"].cpu().numpy().view(np.uint32).copy()
    q = m._ps["q_slots"].cpu().numpy().view(np.uint64).reshape(2, QCAP, SLOT_STRIDE).copy()
    return ctl, [int(ctl[ctl_head(k)]) for k in (0, 1)], [int(ctl[ctl_tail(k)]) for k in (0, 1)], q


def totals_of(m):
    import torch
    torch.cuda.synchronize()
    return m._ps["totals"].cpu().numpy().astype(np.int64).copy()


def check(heads, tails, entries, d_totals, n_slots, servers):
    """The rings of ONE launch that did not give up.  d_totals: the launch's own counts (totals after - before); n_slots:
    the launch's game slots; servers: the workgroups that served the rings.

      * tails match the totals: send_request counts every request it reserves an entry for;
      * entries are well formed: in every slot a ticket below the tail maps to, the WORDS granules carry the tag of the
        LAST such ticket, the kind bit is the ring's, the game is NOBODY or a slot of the launch, the unused granules
        are 0; a slot no ticket reached is all 0;
      * heads against tails: every policy request is waited for, so a ticket was handed out for each; value entries
        without a ticket are at most the requests nobody waits for;
      * no workgroup holds more than one unserved ticket: the tickets beyond the tails number at most `servers`;
      * a pair walk takes two value entries."""
    d = np.asarray(d_totals, dtype=np.int64)
    entries = np.asarray(entries, dtype=np.uint64).reshape(2, QCAP, SLOT_STRIDE)
    assert tails[KIND_VALUE] == d[T_VALUE] + d[T_AHEAD], ("value tail", tails[KIND_VALUE], int(d[T_VALUE]), int(d[T_AHEAD]))
    assert tails[KIND_POLICY] == d[T_POLICY], ("policy tail", tails[KIND_POLICY], int(d[T_POLICY]))
    for q in (KIND_VALUE, KIND_POLICY):
        ring, tail = entries[q], tails[q]
        reached = min(tail, QCAP)
        assert not ring[reached:].any(), "ring %d: a slot no ticket reached is not zero" % q
        if reached == 0:
            continue
        slots = np.arange(reached, dtype=np.int64)
        want = slots + (tail - 1 - slots) // QCAP * QCAP + 1           # last_ticket(slot, tail) + 1
        tags = (ring[:reached, :WORDS] >> np.uint64(32)).astype(np.int64)
        bad = np.nonzero((tags != want[:, None]).any(axis=1))[0]
        assert len(bad) == 0, "ring %d: %d entries do not carry their last ticket's tag (first: slot %d, tags %s, want %d)" % (
            q, len(bad), int(bad[0]), tags[bad[0]].tolist(), int(want[bad[0]]))
        assert not ring[:reached, WORDS:].any(), "ring %d: an unused granule was written" % q
        who = (ring[:reached, W_WHO] & LOW).astype(np.int64)
        assert np.all(who >> 31 == q), "ring %d: an entry of the other kind" % q
        game = who & 0x7FFFFFFF
        assert np.all((game == NOBODY) | (game < n_slots)), "ring %d: a game beyond the launch's %d slots" % (q, n_slots)
        if q == KIND_POLICY:
            assert np.all(game != NOBODY), "a policy request nobody waits for"
    assert heads[KIND_POLICY] >= tails[KIND_POLICY], ("policy entries without a ticket", heads[KIND_POLICY], tails[KIND_POLICY])
    assert tails[KIND_VALUE] - heads[KIND_VALUE] <= d[T_AHEAD], ("value entries without a ticket", heads[KIND_VALUE],
                                                                tails[KIND_VALUE], int(d[T_AHEAD]))
    beyond = sum(max(0, heads[q] - tails[q]) for q in (KIND_VALUE, KIND_POLICY))
    assert beyond <= servers, ("tickets beyond the tails", beyond, servers)
    assert 0 <= d[T_PAIRS] <= tails[KIND_VALUE] // 2, ("pair walks", int(d[T_PAIRS]), tails[KIND_VALUE])
    return dict(heads=list(heads), tails=list(tails), beyond=beyond, pairs=int(d[T_PAIRS]), ahead=int(d[T_AHEAD]))


def audit(m, totals_before, game_wgs_serve=None):
    """check() of engine m's rings after its last launch.  totals_before: totals_of(m) before that launch.
    game_wgs_serve: the game workgroups that serve the rings once their games are done -- default: those of the launch
    (ctl[CTL_FINISHED]: all of them, in a launch that did not give up), none in the role split, whose game launch ends
    instead; the arena passes both agents' (a game workgroup of either serves both)."""
    ctl, heads, tails, entries = read(m)
    assert int(ctl[CTL_ABORT]) == 0, "the launch gave up: nothing to audit"
    if game_wgs_serve is None:
        game_wgs_serve = 0 if getattr(m, "_split", None) is not None else int(ctl[CTL_FINISHED])
    n_slots = m.n_games * (m.wave if getattr(m, "wave_entry", False) else 1)
    return check(heads, tails, entries, totals_of(m) - np.asarray(totals_before, dtype=np.int64), n_slots,
                 int(ctl[CTL_NET_WGS]) + int(game_wgs_serve))
