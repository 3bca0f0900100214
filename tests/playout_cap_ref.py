"""The rule of playout-cap randomisation (include/iago_hip_serving.h, iago_mcts_search_cap) in a few lines of numpy, on
the oracle's Philox (pinned to the Random123 vectors in test_oracle_golden.py).  At a searched turn t (the game's turn
counter, passes included) of the game with global id G:

    w       word t & 3 of Philox4x32-10 on the counter (G, t >> 2, 0, 0), key = seed with its high word ^ 0x43415050
    full    (w >> 24) < full_per_256          (full_per_256 in 1 .. 256)
    budget  n_sims on a full turn, n_fast on a fast one; valid 1 / 4"""
from oracle import oracle as orc

CAP_KEY = 0x43415050   # "CAPP"


def word(seed, game_id, turn):
    """The raw 32-bit word of (seed, global game id, turn)."""
    key = (int(seed) ^ (CAP_KEY << 32)) & 0xFFFFFFFFFFFFFFFF
    return int(orc.philox(key, int(game_id) & 0xFFFFFFFF, int(turn) >> 2, 0, 0)[int(turn) & 3])


def is_full(seed, game_id, turn, full_per_256):
    assert 1 <= full_per_256 <= 256
    return (word(seed, game_id, turn) >> 24) < full_per_256


def valid_code(seed, game_id, turn, full_per_256):
    return 1 if is_full(seed, game_id, turn, full_per_256) else 4


def budget(seed, game_id, turn, full_per_256, n_sims, n_fast):
    assert 1 <= n_fast <= n_sims
    return n_sims if is_full(seed, game_id, turn, full_per_256) else n_fast
