"""The root split of the exact endgame solver (include/iago_hip_serving.h, iago_solve_endgame_split) in a few lines of
Python, on top of endgame_ref.py and lane_search_ref.py.

A node (own, opp) with k split plies left (the root: split, 1 or 2)

    is a JOB (own, opp)      when k == 0 or its mover has no legal move -- it must pass, or the game is over: its
                             (score, move, nodes) are what iago_solve_endgame returns for that position
                             (lane_search_ref.solve), found with the full window on a stack of its own empties;
    is EXPANDED otherwise:   its children are its legal moves in ascending index, each with k - 1; its value is the
                             maximum of the negated children's values.

So a root that must pass or whose game is over is its own job (its move the job's, -1 / -2), and a root with fewer
empties than split plies ends in finished-game jobs.  The root's move is the lowest-indexed move whose value equals the
score, its best set every move whose value does, its row every first move's value.  The jobs of a root are listed in
canonical order: first move ascending, then second move ascending.  nodes = the nodes expanded (the root, and every
child with a second move below it; none when the root is the job) + the sum of the jobs' nodes."""
from . import endgame_moves_ref as mr
from . import lane_search_ref as ls
from .endgame_ref import bit_legal, empties, late_positions

NO_MOVE = -128   # IAGO_ENDGAME_NO_MOVE


def check_split(split):
    if isinstance(split, bool) or split not in (1, 2):
        raise ValueError("split must be 1 or 2, not %r" % (split,))


def moves_of(own, opp):
    legal = bit_legal(own, opp)
    return [m for m in range(64) if legal >> m & 1]


def jobs_of(own, opp, split):
    """The jobs of one root in canonical order: [(own, opp, the job's empties, first move, second move)], -1 for a
    move the path does not have."""
    check_split(split)
    out = []

    def walk(a, b, k, path):
        moves = moves_of(a, b)
        if k == 0 or not moves:
            out.append((a, b, empties(a, b)) + tuple(path + [-1] * (2 - len(path))))
            return
        for m in moves:
            walk(*ls._play(a, b, m), k - 1, path + [m])

    walk(int(own), int(opp), split, [])
    return out


def expanded_of(jobs):
    """The nodes a root's split expanded: none when the root is the job, else the root and every child with a second
    move below it."""
    if jobs[0][3] < 0:
        return 0
    return 1 + len({j[3] for j in jobs if j[4] >= 0})


def combine(jobs, values):
    """(score, move, best set, {first move: value}) of a root from its jobs (canonical order) and their (score, move)
    values: the jobs minimaxed back, the sign turned once per ply of the path.  A root that is its own job: the job's
    score and move, the empty set, no values."""
    if jobs[0][3] < 0:
        return values[0][0], values[0][1], 0, {}
    child = {}   # first move -> the child's value from the child's mover's view
    for (_, _, _, m1, m2), v in zip(jobs, values):
        if m2 < 0:
            child[m1] = v[0]
        else:
            child[m1] = max(child.get(m1, -100), -v[0])
    row = {m1: -v for m1, v in child.items()}
    score = max(row.values())
    best = sum(1 << m for m, v in row.items() if v == score)
    return score, ls._lowest(best), best, row


def split_solve(own, opp, split, wld=False):
    """What iago_solve_endgame_split answers for one admitted root: a dict of score, move, nodes, best, row (the 64
    cells of move_score), jobs and job_values [(score, move, nodes)]."""
    jobs = jobs_of(own, opp, split)
    values = [ls.solve(a, b, wld) for a, b, _, _, _ in jobs]
    score, move, best, row = combine(jobs, values)
    return dict(score=score, move=move, best=best, row=[row.get(a, NO_MOVE) for a in range(64)], jobs=jobs,
                job_values=values, nodes=expanded_of(jobs) + sum(v[2] for v in values))


def child_must_pass():
    """A root of 5 empties with a child (after move 63) that must pass while the game goes on, beside expanded
    children."""
    own, opp = late_positions(64, 77, 3, 8)
    for a, b in zip(own, opp):
        if "child_pass" in kinds_of(int(a), int(b)):
            return int(a), int(b)
    raise AssertionError("no such position")


def kinds_of(own, opp):
    """The job kinds a root shows under split 2, as a set of names."""
    jobs = jobs_of(own, opp, 2)
    out = {"empties%d" % empties(own, opp)} if empties(own, opp) <= 2 else set()
    if jobs[0][3] < 0:
        out.add("root_pass" if bit_legal(jobs[0][1], jobs[0][0]) else "root_over")
        return out
    for a, b, _, m1, m2 in jobs:
        if m2 < 0:
            out.add("child_pass" if bit_legal(b, a) else "child_over")
        else:
            out.add("two_ply")
    row = combine(jobs, [ls.solve(a, b) for a, b, _, _, _ in jobs])[3]
    if list(row.values()).count(max(row.values())) > 1:
        out.add("tie")
    return out


KINDS = {"root_pass", "root_over", "child_pass", "child_over", "two_ply", "tie", "empties0", "empties1", "empties2"}


def position_set(n=48, hi=8, seed=41):
    """n late positions of 0 .. hi empties, endgame_moves_ref's hand-made roots and child_must_pass(): two lists of
    Python ints."""
    own, opp = late_positions(n, seed, 0, hi)
    own, opp = [int(a) for a in own], [int(b) for b in opp]
    for _, a, b in mr.hand_made():
        own.append(a)
        opp.append(b)
    a, b = child_must_pass()
    return own + [a], opp + [b]
