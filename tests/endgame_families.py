"""The position families of tests/golden/endgame_deep.json: what makes a row a member of its family, checked by the
generator (tests/golden/make_endgame_golden.py) when it picks rows and by tests/test_endgame_ref_cpu.py on the
committed fixture, so that a family cannot silently degrade into ordinary positions.  Rules: the bitboard twin of
tests/endgame_ref.py; values: the C reference (oracle.solve_endgame / root_values).  Also the 8 board symmetries."""
from oracle import oracle as orc

from . import endgame_ref as ref

FAMILIES = ("random", "sparse", "pass2", "rootpass", "passend", "over", "over1", "ties", "sym")
SCORE_FAMILIES_EMPTIES = 8   # "early end": at least this many empties left when the game ends


def popcount(x):
    return bin(int(x)).count("1")


def principal_line(own, opp):
    """[(ply, kind, empties)] along a line of best play (the reference's move at every node), kind = 'move', 'pass'
    or 'end' (the last entry, with the empties left)."""
    own, opp, ply, line = int(own), int(opp), 0, []
    while True:
        e = ref.empties(own, opp)
        if ref.bit_legal(own, opp) == 0:
            if ref.bit_legal(opp, own) == 0:
                line.append((ply, "end", e))
                return line
            line.append((ply, "pass", e))
            own, opp = opp, own
        else:
            m = orc.solve_endgame(own, opp)[1]
            line.append((ply, "move", e))
            own, opp = ref.BitRules.play((own, opp), m)
        ply += 1


def is_sparse(r):
    """One side has at most 8 stones (so few empties can ever be played), there is a tree to search all the same."""
    few = min(popcount(r["own"]), popcount(r["opp"])) <= 8
    return few and r["empties"] >= 17 and r["exact"][1] >= -1 and r["exact"][2] >= 20


def is_pass2(r):
    return sum(1 for _, kind, _ in principal_line(r["own"], r["opp"]) if kind == "pass") >= 2


def is_rootpass(r):
    if r["exact"][1] != -1:
        return False
    vals = orc.root_values(r["opp"], r["own"])
    return sum(1 for v in vals.values() if v == max(vals.values())) >= 2


def is_passend(r):
    line = principal_line(r["own"], r["opp"])
    kinds = [k for _, k, _ in line]
    return len(kinds) >= 3 and kinds[-3:] == ["pass", "move", "end"]


def is_over(r):
    """Game over at the root; early (>= 8 empties) unless it is one of the +64 / -64 / 0 full-board rows."""
    own, opp = r["own"], r["opp"]
    if r["empties"] <= 1:
        return abs(r["exact"][0]) == 64 or (r["exact"][0] == 0 and r["empties"] == 0)
    return (ref.bit_legal(own, opp) == 0 and ref.bit_legal(opp, own) == 0 and r["exact"][1] == -2 and
            r["empties"] >= SCORE_FAMILIES_EMPTIES)


def is_over1(r):
    """Some root move ends the game one ply below the root with >= 8 empties left."""
    own, opp = r["own"], r["opp"]
    for m in ref.BitRules.moves((own, opp)):
        a, b = ref.BitRules.play((own, opp), m)
        if ref.bit_legal(a, b) == 0 and ref.bit_legal(b, a) == 0 and ref.empties(a, b) >= SCORE_FAMILIES_EMPTIES:
            return True
    return False


def first_by_fewest_replies(own, opp):
    """The root move a fewest-replies-first order (ties: the lowest index) tries first."""
    def replies(m):
        a, b = ref.BitRules.play((own, opp), m)
        return popcount(ref.bit_legal(a, b))
    return min(ref.BitRules.moves((own, opp)), key=lambda m: (replies(m), m))


def optimal_moves(values):
    vals = {int(m): v for m, v in values.items()}
    top = max(vals.values())
    return sorted(m for m, v in vals.items() if v == top)


def is_tie(r):
    if not r["values"]:
        return False
    best = optimal_moves(r["values"])
    return len(best) >= 3 and best[0] != first_by_fewest_replies(r["own"], r["opp"])


def is_sym(r):
    return bool(r["values"]) and 12 <= r["empties"] <= 16 and r["exact"][1] == optimal_moves(r["values"])[0]


CHECKS = dict(random=lambda r: 11 <= r["empties"] <= 20, sparse=is_sparse, pass2=is_pass2, rootpass=is_rootpass,
              passend=is_passend, over=is_over, over1=is_over1, ties=is_tie, sym=is_sym)


def check_fixture(fx):
    """Every row is what its family says, every family is there, every empties count 11 .. 20 has its rows in both
    modes, no row is above the node cap."""
    rows = fx["rows"]
    for r in rows:
        assert CHECKS[r["family"]](r), (r["family"], hex(r["own"]), hex(r["opp"]))
        assert r["empties"] == ref.empties(r["own"], r["opp"]) <= 20 and r["own"] & r["opp"] == 0
        assert r["exact"] or r["wld"]
        for mode in ("exact", "wld"):
            assert r[mode] is None or max(r[mode][2:]) <= fx["n_cap"]
        if r["exact"] and r["wld"]:
            assert r["wld"][0] == (r["exact"][0] > 0) - (r["exact"][0] < 0)
    assert {r["family"] for r in rows} == set(FAMILIES)
    for e in range(11, 21):
        for mode in ("exact", "wld"):
            n = sum(1 for r in rows if r["empties"] == e and r[mode])
            assert n >= fx["rows_min"], (e, mode, n)
    over = {r["exact"][0] for r in rows if r["family"] == "over"}
    assert {64, -64, 0} <= over
    assert sum(1 for r in rows if r["family"] == "sym") >= 64
    assert max(r["empties"] for r in rows if r["family"] == "sparse") == 20


# ------------------------------------------------------------------ the 8 symmetries of the board
def _cell(k, a):
    r, c = a // 8, a % 8
    if k & 1:
        c = 7 - c      # mirror left-right
    if k & 2:
        r = 7 - r      # mirror top-bottom
    if k & 4:
        r, c = c, r    # transpose
    return 8 * r + c


def sym_move(k, a):
    """Where symmetry k (0 .. 7) takes square a."""
    return _cell(k, a)


def sym_bits(k, x):
    x, out = int(x), 0
    for a in range(64):
        if (x >> a) & 1:
            out |= 1 << _cell(k, a)
    return out
