"""tests/ring_util.py on hand-built rings: slot_of / last_ticket, the entry's and the reply's coding, and that check()
passes a consistent pair of rings and objects to each kind of damage -- the "test of the test" of
tests/test_request_rings_gpu.py, which must not break the protocol on the device."""
import numpy as np
import pytest

from tests import ring_util as ru

OWN, OPP = 0x0000000810000000, 0x8000001008000001       # (opp: both halves' top and bottom bits in use)


def test_slot_and_last_ticket():
    assert ru.slot_of(0) == 0 and ru.slot_of(ru.QCAP - 1) == ru.QCAP - 1 and ru.slot_of(ru.QCAP) == 0
    assert ru.slot_of(3 * ru.QCAP + 17) == 17
    assert ru.last_ticket(0, 0) is None and ru.last_ticket(5, 5) is None
    assert ru.last_ticket(5, 6) == 5 and ru.last_ticket(0, ru.QCAP) == 0
    assert ru.last_ticket(0, ru.QCAP + 1) == ru.QCAP                # the ring wrapped: slot 0 holds ticket QCAP
    assert ru.last_ticket(1, ru.QCAP + 1) == 1
    assert ru.last_ticket(17, 3 * ru.QCAP + 17) == 2 * ru.QCAP + 17
    for tail in (1, 7, ru.QCAP, ru.QCAP + 3, 2 * ru.QCAP + 1):      # against the definition, ticket by ticket
        last = {}
        for t in range(tail):
            last[ru.slot_of(t)] = t
        for s in (0, 1, 2, 6, 7, ru.QCAP - 1):
            assert ru.last_ticket(s, tail) == last.get(s)


def test_entry_and_reply_coding():
    e = ru.entry(41, ru.KIND_POLICY, 1234, 0xCAFEF00D, OWN, OPP)
    assert e.dtype == np.uint64 and e.shape == (ru.SLOT_STRIDE,)
    assert int(e[ru.W_WHO]) == (42 << 32) | (1 << 31) | 1234
    assert int(e[ru.W_OPP_HI]) == (42 << 32) | 0x80000010 and int(e[ru.W_OWN_LO]) == (42 << 32) | 0x10000000
    assert not e[ru.WORDS:].any()
    d = ru.decode(e)
    assert d == dict(tags=[42] * ru.WORDS, kind=ru.KIND_POLICY, game=1234, tag=0xCAFEF00D, own=OWN, opp=OPP)
    d = ru.decode(ru.entry(0xFFFFFFFE, ru.KIND_VALUE, ru.NOBODY, 7, OPP, OWN))
    assert d["tags"] == [0xFFFFFFFF] * ru.WORDS and d["kind"] == ru.KIND_VALUE and d["game"] == ru.NOBODY
    assert (d["own"], d["opp"]) == (OPP, OWN)
    x = ru.reply_word(0xCAFEF00D, 0xBF800000)
    assert x == 0xCAFEF00DBF800000 and ru.reply_tag(x) == 0xCAFEF00D and ru.reply_bits(x) == 0xBF800000


N_SLOTS = 16


def _rings(n_value, n_policy, n_nobody=0):
    """Rings as a launch of N_SLOTS game slots leaves them: n_value requests of games and n_nobody of nobody in the value
    ring (nobody's last), n_policy in the policy ring; every ticket handed out; the totals to match."""
    q = np.zeros((2, ru.QCAP, ru.SLOT_STRIDE), np.uint64)
    for t in range(n_value + n_nobody):
        game = t % N_SLOTS if t < n_value else ru.NOBODY
        q[ru.KIND_VALUE, ru.slot_of(t)] = ru.entry(t, ru.KIND_VALUE, game, 100 + t, OWN + t, OPP)
    for t in range(n_policy):
        q[ru.KIND_POLICY, ru.slot_of(t)] = ru.entry(t, ru.KIND_POLICY, t % N_SLOTS, 200 + t, OWN, OPP + 2 * t)
    tails = [n_value + n_nobody, n_policy]
    d = np.zeros(17, np.int64)
    d[ru.T_VALUE], d[ru.T_POLICY], d[ru.T_AHEAD], d[ru.T_PAIRS] = n_value, n_policy, n_nobody, (n_value + n_nobody) // 2
    return list(tails), tails, q, d


def test_check_passes_consistent_rings():
    heads, tails, q, d = _rings(37, 9, 4)
    got = ru.check(heads, tails, q, d, N_SLOTS, servers=3)
    assert got["tails"] == [41, 9] and got["beyond"] == 0 and got["pairs"] == 20
    # tickets beyond the tails, one per server; value entries of nobody left without a ticket; no pair walk at all
    d[ru.T_PAIRS] = 0
    assert ru.check([41 - 4, 9 + 3], tails, q, d, N_SLOTS, servers=3)["beyond"] == 3
    assert ru.check([41 + 2, 9 + 1], tails, q, d, N_SLOTS, servers=3)["beyond"] == 3
    # a ring that wrapped: slot s holds its LAST ticket's entry
    heads, tails, q, d = _rings(ru.QCAP + 5, 1)
    assert ru.decode(q[ru.KIND_VALUE, 4])["tags"] == [ru.QCAP + 5] * ru.WORDS
    assert ru.decode(q[ru.KIND_VALUE, 5])["tags"] == [6] * ru.WORDS
    ru.check(heads, tails, q, d, N_SLOTS, servers=1)
    # empty rings
    heads, tails, q, d = _rings(0, 0)
    ru.check(heads, tails, q, d, N_SLOTS, servers=1)


def _damaged(what):
    heads, tails, q, d = _rings(37, 9, 4)
    heads = list(heads)
    servers = 3
    if what == "value tail above the count":
        d[ru.T_VALUE] -= 1
    elif what == "policy tail below the count":
        d[ru.T_POLICY] += 1
    elif what == "one word of an entry is an older ticket's":
        q[ru.KIND_VALUE, 7, ru.W_OPP_LO] = ru.entry_word(6, 1)
    elif what == "an entry was never written":
        q[ru.KIND_POLICY, 8] = 0
    elif what == "the who word came before the others":            # (tag of the ticket, the rest still zero)
        q[ru.KIND_VALUE, 3, 1:] = 0
    elif what == "an entry of the other kind":
        q[ru.KIND_VALUE, 2] = ru.entry(2, ru.KIND_POLICY, 2, 102, OWN, OPP)
    elif what == "a game beyond the slots":
        q[ru.KIND_POLICY, 2] = ru.entry(2, ru.KIND_POLICY, N_SLOTS, 202, OWN, OPP)
    elif what == "a policy request of nobody":
        q[ru.KIND_POLICY, 2] = ru.entry(2, ru.KIND_POLICY, ru.NOBODY, 202, OWN, OPP)
    elif what == "an entry beyond the tail":
        q[ru.KIND_POLICY, 9] = ru.entry(9, ru.KIND_POLICY, 1, 209, OWN, OPP)
    elif what == "an unused granule written":
        q[ru.KIND_VALUE, 0, ru.WORDS] = 1
    elif what == "a policy entry without a ticket":
        heads[ru.KIND_POLICY] -= 1
    elif what == "a waited-for value entry without a ticket":
        heads[ru.KIND_VALUE] -= 5
    elif what == "two unserved tickets in one workgroup":
        heads[ru.KIND_VALUE] += 2
        heads[ru.KIND_POLICY] += 2
    elif what == "more pair walks than pairs":
        d[ru.T_PAIRS] = 21
    else:
        raise KeyError(what)
    return heads, tails, q, d, servers


DAMAGE = ["value tail above the count", "policy tail below the count", "one word of an entry is an older ticket's",
          "an entry was never written", "the who word came before the others", "an entry of the other kind",
          "a game beyond the slots", "a policy request of nobody", "an entry beyond the tail", "an unused granule written",
          "a policy entry without a ticket", "a waited-for value entry without a ticket",
          "two unserved tickets in one workgroup", "more pair walks than pairs"]


@pytest.mark.parametrize("what", DAMAGE)
def test_check_objects_to_damage(what):
    heads, tails, q, d, servers = _damaged(what)
    with pytest.raises(AssertionError):
        ru.check(heads, tails, q, d, N_SLOTS, servers)
