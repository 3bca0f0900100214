/*
 * oracle/endgame_oracle.c -- TEST INFRASTRUCTURE ONLY.
 *
 * An exact Othello endgame solver to hold iago_solve_endgame (include/iago_hip_serving.h) against at the depths the
 * Python references of tests/endgame_ref.py cannot reach.  Original to this repository (the project this one was
 * modelled on has no solver); it shares no code with iago_amd/csrc and is meant to be trusted by reading:
 *   * its own rules on two 64-bit sets (own = the side to move, bit a = row * 8 + col): a legal-move flood and a
 *     ray walk for the flips, both plain shift-and-mask loops over the 8 directions;
 *   * a recursive fail-soft negamax alpha-beta, no explicit stack, no hash table, no parity tricks;
 *   * game: a side without a move passes, the game ends when neither side can move, score = #own - #opp with the
 *     empty squares for nobody; wld scores the end by its sign;
 *   * order: at nodes with more than ORDER_EMPTIES empties the move with the fewest replies goes first (ties: the
 *     lower index).  The VALUE does not depend on the order; the root's MOVE does not either: the root tries its
 *     moves in ascending index and a later move must beat the best strictly, so the lowest index reaching the
 *     score wins.  (Asked to, the root orders its moves like an inner node and keeps ties of a lower index exact:
 *     the same answer from another tree, whose node count tells what a solver with such a root has to visit.)
 * A node budget (limit > 0) lets a caller give up on a position that is too heavy: the search unwinds and the
 * entry point returns ORC_ENDGAME_ABORTED.
 *
 * Pinned on the CPU to both Python references and to hand-built positions (tests/test_endgame_ref_cpu.py).
 */
#include <stdint.h>

#define ORC_API __attribute__((visibility("default")))

#define ORDER_EMPTIES 6
#define INF 1000
#define ORC_ENDGAME_ABORTED (-1000)

#define NOT_A 0xFEFEFEFEFEFEFEFEull /* every square but file a (col 0) */
#define NOT_H 0x7F7F7F7F7F7F7F7Full /* every square but file h (col 7) */

/* one step in direction k: east, west, south, north, south-east, south-west, north-east, north-west */
static inline __attribute__((always_inline)) uint64_t step(uint64_t x, int k)
{
    switch (k) {
    case 0: return (x & NOT_H) << 1;
    case 1: return (x & NOT_A) >> 1;
    case 2: return x << 8;
    case 3: return x >> 8;
    case 4: return (x & NOT_H) << 9;
    case 5: return (x & NOT_A) << 7;
    case 6: return (x & NOT_H) >> 7;
    default: return (x & NOT_A) >> 9;
    }
}

static int popcount(uint64_t x) { return __builtin_popcountll(x); }

/* the empty squares where `own` brackets a run of `opp` */
static uint64_t legal_moves(uint64_t own, uint64_t opp)
{
    const uint64_t empty = ~(own | opp);
    uint64_t legal = 0;
#pragma GCC unroll 8
    for (int k = 0; k < 8; k++) {
        uint64_t run = step(own, k) & opp;
        for (int i = 0; i < 5; i++)
            run |= step(run, k) & opp;
        legal |= step(run, k) & empty;
    }
    return legal;
}

/* the stones of `opp` that a stone of `own` on square m turns over */
static uint64_t flips(uint64_t own, uint64_t opp, int m)
{
    uint64_t all = 0;
#pragma GCC unroll 8
    for (int k = 0; k < 8; k++) {
        uint64_t x = step(1ull << m, k), run = 0;
        while (x & opp) {
            run |= x;
            x = step(x, k);
        }
        if (x & own)
            all |= run;
    }
    return all;
}

typedef struct {
    int wld;
    int aborted;
    int64_t nodes;
    int64_t limit; /* <= 0: none */
    int fastest_root;
} ctx_t;

static int final_score(uint64_t own, uint64_t opp, int wld)
{
    const int d = popcount(own) - popcount(opp);
    return wld ? (d > 0) - (d < 0) : d;
}

/* the legal moves of (own, opp) in the order they are tried; returns their number */
static int ordered_moves(uint64_t own, uint64_t opp, uint64_t legal, int *out)
{
    int n = 0, key[64];
    const int order = 64 - popcount(own | opp) > ORDER_EMPTIES;
    for (int m = 0; m < 64; m++) {
        if (!((legal >> m) & 1))
            continue;
        int k = 0;
        if (order) {
            const uint64_t f = flips(own, opp, m);
            k = popcount(legal_moves(opp & ~f, own | f | (1ull << m)));
        }
        int i = n++;
        while (i > 0 && key[i - 1] > k) { /* insertion: stable, so equal keys stay in ascending index */
            key[i] = key[i - 1];
            out[i] = out[i - 1];
            i--;
        }
        key[i] = k;
        out[i] = m;
    }
    return n;
}

/* fail-soft: exact inside (alpha, beta), a bound outside */
static int search(ctx_t *c, uint64_t own, uint64_t opp, int alpha, int beta, int passed)
{
    if (!passed)
        c->nodes++; /* (a pass stays at its node) */
    if (c->limit > 0 && c->nodes > c->limit)
        c->aborted = 1;
    if (c->aborted)
        return 0;
    const uint64_t legal = legal_moves(own, opp);
    if (legal == 0) {
        if (passed || legal_moves(opp, own) == 0)
            return final_score(own, opp, c->wld);
        return -search(c, opp, own, -beta, -alpha, 1);
    }
    int moves[64];
    const int n = ordered_moves(own, opp, legal, moves);
    int best = -INF;
    for (int i = 0; i < n; i++) {
        const uint64_t f = flips(own, opp, moves[i]);
        const int a = alpha > best ? alpha : best;
        const int v = -search(c, opp & ~f, own | f | (1ull << moves[i]), -beta, -a, 0);
        if (v > best) {
            best = v;
            if (best >= beta)
                break;
        }
    }
    return best;
}

/* the root.  Its moves are tried in ascending index, or (c->fastest_root) in the order of every other node.  A move
 * of a lower index than the best so far is searched with a window that keeps a tie exact (best - 1), a higher one
 * must beat the best strictly: so *move is the lowest index reaching the score in either order (in ascending order
 * every later move has the higher index).  values[] (if given) gets every move's exact value instead (full window).
 * The expected results of the tests always come from the ascending path; the ordered path is asked for node counts
 * only and has to give the same score and move.  Returns the score; *move as the header says. */
static int root(ctx_t *c, uint64_t own, uint64_t opp, int *move, int *moves_out, int *values_out, int *n_out)
{
    const int hi = c->wld ? 1 : 64, lo = -hi; /* no value lies outside [lo, hi]: this window is exact */
    uint64_t legal = legal_moves(own, opp);
    int sign = 1;
    *move = 0;
    if (n_out)
        *n_out = 0;
    c->nodes++;
    if (legal == 0) {
        legal = legal_moves(opp, own);
        if (legal == 0) {
            *move = -2;
            return final_score(own, opp, c->wld);
        }
        const uint64_t t = own; /* the side to move passes: the opponent's best, negated */
        own = opp;
        opp = t;
        sign = -1;
        *move = -1;
    }
    int moves[64], n_moves = 0;
    if (c->fastest_root && !values_out)
        n_moves = ordered_moves(own, opp, legal, moves);
    else
        for (int m = 0; m < 64; m++)
            if ((legal >> m) & 1)
                moves[n_moves++] = m;
    int best = -INF, best_move = 64, n = 0;
    for (int i = 0; i < n_moves; i++) {
        const int m = moves[i];
        int a = lo;
        if (!values_out && best > -INF)
            a = m < best_move ? best - 1 : best;
        if (a >= hi)
            continue; /* nothing can beat the best, and this move cannot tie it with a lower index */
        const uint64_t f = flips(own, opp, m);
        const int v = -search(c, opp & ~f, own | f | (1ull << m), -hi, -(a > lo ? a : lo), 0);
        if (c->aborted)
            return 0;
        if (values_out && sign == 1) {
            moves_out[n] = m;
            values_out[n] = v;
            n++;
        }
        if (v > best || (v == best && m < best_move)) {
            best = v;
            best_move = m;
        }
    }
    if (sign == 1)
        *move = best_move;
    if (n_out)
        *n_out = n;
    return sign * best;
}

/* score of (own, opp), own to move; *move: the lowest-indexed move reaching it, -1 = must pass, -2 = game over.
 * limit > 0: give up after that many nodes (returns ORC_ENDGAME_ABORTED).  fastest_root: the root's moves in the
 * order of the inner nodes (same result, another tree: what a solver that orders its root so has to visit). */
ORC_API int orc_endgame_solve(uint64_t own, uint64_t opp, int wld, int64_t limit, int fastest_root, int *move,
                              int64_t *nodes)
{
    ctx_t c = {wld != 0, 0, 0, limit, fastest_root != 0};
    const int s = root(&c, own, opp, move, 0, 0, 0);
    *nodes = c.nodes;
    return c.aborted ? ORC_ENDGAME_ABORTED : s;
}

/* every root move (ascending) with its exact value, each searched with the full window; returns their number (0
 * when the side to move has no move), or ORC_ENDGAME_ABORTED. */
ORC_API int orc_endgame_root_values(uint64_t own, uint64_t opp, int wld, int64_t limit, int *moves, int *values,
                                    int64_t *nodes)
{
    ctx_t c = {wld != 0, 0, 0, limit, 0};
    int move, n;
    root(&c, own, opp, &move, moves, values, &n);
    *nodes = c.nodes;
    return c.aborted ? ORC_ENDGAME_ABORTED : n;
}
