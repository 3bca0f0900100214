"""Host reference of iago_play_endgame: a game played from a late position to its end under perfect play.

Both sides play endgame_ref.solve_bits' move (EXACT: the lowest-indexed move reaching the best final disc difference)
at every turn that is theirs to move; the turn structure and the books are the reference's game loop as the engine's
whole-game paths keep them (game.py:32,117-142,253-255): stone_num counts a stone per move, a pass after a pass sets
it to 64, `while stone_num < 64` is tested once per pair of turns -- after the odd turn --, and the game ends at an even
turn or at max_turns.  Positions are (own, opp) Python ints, own = the side to move, bit a = row*8+col.
"""
from . import endgame_ref as ref

_solved = {}


def solve(own, opp):
    """endgame_ref.solve_bits(own, opp), remembered: a game's positions are solved once however often it is replayed
    with other books."""
    key = (int(own), int(opp))
    if key not in _solved:
        _solved[key] = ref.solve_bits(*key)
    return _solved[key]


def play_out(own, opp, turn, stones, pass_flg, max_turns, solve=solve):
    """The game from (own, opp) at turn `turn` with the books (stones, pass_flg), to its end.  Returns dict(rows,
    n_turns, own, opp): rows = [(turn, own, opp, valid, move, score)] for every turn from `turn` on (valid 3: a solved
    move, score its exact final disc difference from the mover's view; valid 0: a pass or no turn, move -1, score 0);
    n_turns the turns the game took; (own, opp) the final position, own = the side that would move next."""
    own, opp, turn, stones, pass_flg = int(own), int(opp), int(turn), int(stones), bool(pass_flg)
    assert 0 <= turn < max_turns and own & opp == 0
    over = False
    rows = []
    while True:
        moved = ref.bit_legal(own, opp) != 0 and not over
        if moved:
            score, move = solve(own, opp)
            rows.append((turn, own, opp, 3, move, score))
            own, opp = ref.BitRules.play((own, opp), move)   # (the stone, the flips, the swap of sides)
        else:
            rows.append((turn, own, opp, 0, -1, 0))
            own, opp = opp, own
        was_over = over
        stones += 1 if moved else 0
        passing = not moved and not was_over
        if passing and pass_flg:
            stones = 64                      # a pass after a pass ends the game
        if not was_over:
            pass_flg = passing
        if turn % 2 == 1:                    # `while stone_num < 64` once per pair of turns
            over = was_over or stones >= 64
        turn += 1
        if turn >= max_turns or (turn % 2 == 0 and over):
            return dict(rows=rows, n_turns=turn, own=own, opp=opp)


def _play_games(games):
    return [play_out(*g) for g in games]


def play_out_many(games, workers=8):
    """[play_out(*g) for g in games] spread over worker processes (fresh interpreters: the caller may hold a HIP
    context).  Games of one position stay together in a worker, which solves that position once."""
    import multiprocessing
    by_position = {}
    for i, g in enumerate(games):
        by_position.setdefault((int(g[0]), int(g[1])), []).append(i)
    groups = list(by_position.values())
    # (the longest solves first: a position's cost grows steeply with its empties)
    groups.sort(key=lambda idx: -ref.empties(games[idx[0]][0], games[idx[0]][1]))
    with multiprocessing.get_context("spawn").Pool(workers) as pool:
        done = pool.map(_play_games, [[tuple(int(x) for x in games[i]) for i in idx] for idx in groups], chunksize=1)
    out = [None] * len(games)
    for idx, res in zip(groups, done):
        for i, r in zip(idx, res):
            out[i] = r
    return out
