"""The root split of the fixed-depth alpha-beta opponent (include/iago_hip_serving.h, iago_alphabeta_moves_split) in a
few lines of Python, on top of alphabeta_ref.py.

A node (own, opp) with d depth left and k split plies left (the root: depth, split; split is 1 or 2 and below depth)

    is a JOB (own, opp, d)   when k == 0 or its mover has no legal move: its value is search(own, opp, d) from its
                             mover's view -- what iago_alphabeta_moves returns for that position at depth d;
    is EXPANDED otherwise:   its children are its legal moves in ascending index, each with (d - 1, k - 1); its value
                             is the maximum of the negated children's values.

So a root that must pass or whose game is over is one job of the full depth (its move the job's, -1 / -2), a child that
cannot move is one job of depth - 1, and every other job has depth - split left.  The root's move is the lowest-indexed
move whose value equals the score.  The jobs of a root are listed in canonical order: first move ascending, then second
move ascending.  nodes = the nodes expanded + the sum of the jobs' nodes."""
from . import alphabeta_ref as ab


def check_split(depth, split):
    if split not in (1, 2) or not 1 <= split <= depth - 1:
        raise ValueError("split must be 1 or 2 and at most depth - 1: split %r at depth %r" % (split, depth))


def jobs_of(own, opp, depth, split):
    """The jobs of one root in canonical order: [(own, opp, depth left, first move, second move)], -1 for a move the
    path does not have."""
    check_split(depth, split)
    own, opp = int(own), int(opp)
    out = []

    def walk(a, b, d, k, path):
        moves = ab.moves_of(a, b)
        if k == 0 or not moves:
            out.append((a, b, d) + tuple(path + [-1] * (2 - len(path))))
            return
        for m in moves:
            walk(*ab.play(a, b, m), d - 1, k - 1, path + [m])

    walk(own, opp, depth, split, [])
    return out


def expanded_of(jobs):
    """The nodes a root's split expanded: none when the root is the job, else the root and every child with a second
    move below it."""
    if jobs[0][3] < 0:
        return 0
    return 1 + len({j[3] for j in jobs if j[4] >= 0})


def combine(jobs, values):
    """(score, move) of a root from its jobs (canonical order) and their (score, move) values: the jobs minimaxed back,
    the sign turned once per ply of the path, the first maximum."""
    if jobs[0][3] < 0:
        return values[0]
    child = {}   # first move -> the child's value from the child's mover's view
    for (_, _, _, m1, m2), (v, _) in zip(jobs, values):
        if m2 < 0:
            child[m1] = v
        else:
            child[m1] = max(child.get(m1, -ab.WINDOW - 1), -v)
    best, best_m = -ab.WINDOW - 1, None
    for m1 in sorted(child):
        if -child[m1] > best:
            best, best_m = -child[m1], m1
    return best, best_m


def split_minimax(own, opp, depth, split):
    """(score, move) of the root through its jobs, every job valued by alphabeta_ref.minimax."""
    jobs = jobs_of(own, opp, depth, split)
    return combine(jobs, [ab.minimax(a, b, d) for a, b, d, _, _ in jobs])


def child_must_pass():
    """A position whose child (after move 47) must pass while the game goes on."""
    from .endgame_ref import late_positions
    o, p = late_positions(16, 0, 2, 12)
    return int(o[4]), int(p[4])


def position_set():
    """alphabeta_ref.position_set() and child_must_pass(): 49 positions, two lists of Python ints."""
    own, opp = ab.position_set()
    a, b = child_must_pass()
    return own + [a], opp + [b]


def job_kinds(jobs):
    """(roots that are jobs themselves, one-ply jobs, two-ply jobs) of a list of jobs."""
    return (sum(1 for j in jobs if j[3] < 0), sum(1 for j in jobs if j[3] >= 0 and j[4] < 0),
            sum(1 for j in jobs if j[4] >= 0))
