// endgame_kernel.hip -- iago_solve_endgame: the exact value of Othello positions with few empties, batched.
//
// Contract: include/iago_hip_serving.h.  The search is lane_search.hpp's -- a lane per position, the node in registers,
// an explicit stack in LDS, passes in place, positions claimed from ctl, the root's tie rule -- on SolverRules below:
//   * a node's remaining levels are its empties, so a lane never holds more frames than the position had empties
//     (28 B per level and lane: alpha / beta / best in 8 bits each);
//   * move order: at nodes with more than ORDER_EMPTIES empties the untried move with the fewest replies for the
//     opponent goes first (fastest first; ties: lowest index), below that index order; a node with one empty is
//     counted directly (the board is full after its move);
//   * mode WLD scores the end of the game by its sign: the same search on values in {-1, 0, 1}, window (-1, 1)
//     around 0 at the root.
// Past time_limit_ms the launch gives up (ctl[0] = 1), every position it has not finished keeps solved = 0.
// iago_solve_endgame_split spreads every root over many lanes with the stages of lane_split.hpp (the ones of
// iago_alphabeta_moves_split): the first one or two plies become JOBS on the device, endgame_jobs_kernel searches a lane
// per job with the full window -- a job's (score, move, nodes) are iago_solve_endgame's on that position -- and a thread
// per root takes the values back, with the set of the best moves and every move's value where they are asked for.
// iago_play_endgame (play_endgame_kernel: one lane per GAME) runs the same search once per turn of a game and plays
// the moves, to the game's end.
#include "abi_common.hpp"
#include "lane_search.hpp"
#include "lane_split.hpp"
#include "othello_dev.hpp"

#include "../../include/iago_hip_serving.h"

using namespace iago;
using namespace iago::lane;

namespace {

constexpr int ORDER_EMPTIES = 6;  // nodes with more empties than this try their moves fastest first

// The final disc difference (wld: its sign); scores are in [-64, 64].  ROOT_: the root's rule (lane_search.hpp).
template <RootRule ROOT_>
struct SolverRulesT {
    static constexpr RootRule ROOT = ROOT_;
    using Info = uint32_t;
    static constexpr int NEG_INF = -100;
    static constexpr bool COUNT_LAST = true;
    static constexpr bool LEAF_CHILDREN = false;
    int32_t wld;

    __device__ __forceinline__ int window() const { return wld ? 1 : 65; }

    __device__ __forceinline__ int terminal(uint64_t own, uint64_t opp) const
    {
        const int d = __popcll(own) - __popcll(opp); // empty squares go to nobody (judge)
        return wld ? (d > 0) - (d < 0) : d;
    }

    // fewest opponent replies first above ORDER_EMPTIES empties, else the lowest index
    __device__ __forceinline__ uint32_t pick_move(uint64_t own, uint64_t opp, uint64_t moves, int empties,
                                                  const ShiftAmounts &SA) const
    {
        return empties > ORDER_EMPTIES ? fewest_replies(own, opp, moves, SA) : lowest_bit(moves);
    }

    // alpha, beta, best in 8 bits each (offset 128), pass flag, move tried
    static __device__ __forceinline__ Info pack(int alpha, int beta, int best, uint32_t passed, uint32_t m)
    {
        return (uint32_t)(alpha + 128) | ((uint32_t)(beta + 128) << 8) | ((uint32_t)(best + 128) << 16) |
               (passed << 24) | (m << 25);
    }

    static __device__ __forceinline__ int unpack(Info info, Search &s)
    {
        s.alpha = (int)(info & 0xFFu) - 128;
        s.beta = (int)((info >> 8) & 0xFFu) - 128;
        s.best = (int)((info >> 16) & 0xFFu) - 128;
        s.passed = (info >> 24) & 1u;
        return (int)(info >> 25);
    }
};

using SolverRules = SolverRulesT<LOWEST>; // iago_solve_endgame, iago_play_endgame

struct EndgameParams {
    const uint64_t *own;
    const uint64_t *opp;
    int64_t n;
    int8_t *score;
    int8_t *move;
    int64_t *nodes;
    uint8_t *solved;
    uint32_t *ctl;
    int32_t wld;
    int32_t max_empties;
    int32_t levels;          // stack frames per lane
    long long clock_limit;   // wall_clock64 ticks (100 MHz)

    __device__ __forceinline__ bool admit(int64_t pos, uint64_t &o, uint64_t &p, int &empties) const
    {
        o = own[pos];
        p = opp[pos];
        empties = 64 - __popcll(o | p);
        if ((o & p) == 0ull && empties <= max_empties)
            return true;
        // refused: solved stays 0
        atomicAdd(&ctl[CTL_REFUSED], 1u);
        score[pos] = 0;
        move[pos] = 0;
        nodes[pos] = 0;
        return false;
    }

    __device__ __forceinline__ void finish(int64_t pos, const Search &s) const
    {
        score[pos] = (int8_t)s.v;
        move[pos] = (int8_t)s.root_move;
        nodes[pos] = s.nodes;
        solved[pos] = 1;
    }
};

__global__ __launch_bounds__(WAVE) void endgame_kernel(EndgameParams P)
{
    extern __shared__ __align__(16) unsigned char stack_lds[];
    search_wave(P, SolverRules{P.wld}, P.n, 0, stack_lds);
}

// iago_solve_endgame_moves: the same launch on the root rules BEST and ALL, with the set of the optimal moves and (ALL)
// the row of per-move values (filled with IAGO_ENDGAME_NO_MOVE before the launch: the search writes the legal moves)
struct MovesParams : EndgameParams {
    uint64_t *best;
    int8_t *move_score;

    __device__ __forceinline__ bool admit(int64_t pos, uint64_t &o, uint64_t &p, int &empties) const
    {
        if (EndgameParams::admit(pos, o, p, empties))
            return true;
        best[pos] = 0ull;
        return false;
    }

    __device__ __forceinline__ void finish(int64_t pos, const Search &s) const
    {
        best[pos] = s.best_set;
        EndgameParams::finish(pos, s);
    }

    __device__ __forceinline__ int8_t *row(int64_t pos) const { return move_score + 64 * pos; }
};

template <RootRule ROOT>
__global__ __launch_bounds__(WAVE) void endgame_moves_kernel(MovesParams P)
{
    extern __shared__ __align__(16) unsigned char stack_lds[];
    search_wave(P, SolverRulesT<ROOT>{P.wld}, P.n, 0, stack_lds);
}

// ---- iago_solve_endgame_split: the stages of lane_split.hpp on the solver's KIND -- a job's levels are its own
// empties, values are int8, the reduction also answers the set of the best moves and every move's value.
struct EmptiesJobs {
    using Score = int8_t;
    static constexpr int NEG_INF = SolverRules::NEG_INF;
    static constexpr bool MOVES = true;
    int32_t max_empties;

    __device__ __forceinline__ bool admits(uint64_t own, uint64_t opp) const
    {
        return (own & opp) == 0ull && 64 - __popcll(own | opp) <= max_empties;
    }
    __device__ __forceinline__ int left(uint64_t own, uint64_t opp, int) const { return 64 - __popcll(own | opp); }
};

// The jobs as the search reads and answers them: positions of an admitted root's subtree, each with its own empties
struct EndgameJobParams {
    const uint64_t *own;
    const uint64_t *opp;
    int8_t *score;
    int8_t *move;
    int64_t *nodes;
    uint8_t *done;
    uint32_t *ctl;
    int32_t wld;
    int32_t levels;          // stack frames per lane: max_empties'
    long long clock_limit;

    __device__ __forceinline__ bool admit(int64_t pos, uint64_t &o, uint64_t &p, int &empties) const
    {
        o = own[pos];
        p = opp[pos];
        empties = 64 - __popcll(o | p); // (at most the root's, which is at most max_empties)
        return true;
    }

    __device__ __forceinline__ void finish(int64_t pos, const Search &s) const
    {
        score[pos] = (int8_t)s.v;
        move[pos] = (int8_t)s.root_move;
        nodes[pos] = s.nodes;
        done[pos] = 1;
    }
};

// over the jobs of a split solve: their number read from ctl (none after an overflow of the job arrays)
__global__ __launch_bounds__(WAVE) void endgame_jobs_kernel(EndgameJobParams P)
{
    extern __shared__ __align__(16) unsigned char stack_lds[];
    const int64_t n = split_jobs_to_claim(P.ctl);
    if ((int64_t)blockIdx.x * WAVE >= n) // nothing to claim: the wave leaves at once
        return;
    search_wave(P, SolverRules{P.wld}, n, 0, stack_lds);
}

// ---- iago_play_endgame: whole games from a late position to their end, both sides solving every turn

struct PlayParams {
    uint64_t *own, *opp;
    int32_t *turn;
    const int32_t *stones;
    const uint8_t *pass_flg, *parked;
    int64_t n, stride;
    uint64_t *rec_own, *rec_opp;
    uint8_t *rec_valid;
    int8_t *rec_move, *rec_score;
    uint8_t *finished;
    uint32_t *ctl;
    int32_t max_turns, max_empties, levels;
    long long clock_limit;
};

// One LANE PER GAME, claimed from the counter: at every turn the mover's position is solved with search_step (EXACT) and
// the move is played with the books of the persistent search's play_move (game.py:117-142,253-255): a stone per move, a
// pass after a pass sets stones = 64, the end of the game is tested once per pair of turns.  TURN: at a turn's start.
// Rules: SolverRules, or (iago_play_endgame_moves, P.rec_best) the root rule BEST: the same move, and the set it is of.
template <class Rules, class Params>
__device__ __forceinline__ void play_endgame_games(const Params &P, unsigned char *stack_lds)
{
    const uint32_t lane = threadIdx.x;
    const Rules R{0};
    const Stack<Rules> K = make_stack<Rules>(stack_lds, P.levels);
    const ShiftAmounts SA = opaque_shift_amounts();
    const long long t0 = wall_clock64();

    Search s = {};
    s.phase = CLAIM;
    int64_t g = 0;
    uint64_t g_own = 0ull, g_opp = 0ull; // the game's position, own = the side to move
    int turn = 0, stones = 0, empties = 0;
    bool pass_flg = false, g_over = false;

    while (true) {
        if (s.phase == CLAIM) {
            if (__hip_atomic_load(&P.ctl[CTL_GAVE_UP], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {
                s.phase = DONE;
            } else {
                g = (int64_t)atomicAdd(&P.ctl[CTL_CLAIM], 1u);
                if (g >= P.n) {
                    s.phase = DONE;
                } else if (P.parked[g] != 0) {
                    g_own = P.own[g];
                    g_opp = P.opp[g];
                    turn = P.turn[g];
                    stones = P.stones[g];
                    pass_flg = P.pass_flg[g] != 0;
                    g_over = false;
                    if ((g_own & g_opp) != 0ull || 64 - __popcll(g_own | g_opp) > P.max_empties || turn < 0 ||
                        turn >= P.max_turns)
                        atomicAdd(&P.ctl[CTL_REFUSED], 1u); // refused: finished stays 0, no row is written
                    else
                        s.phase = TURN;
                }
            }
        }
        if (__builtin_amdgcn_ballot_w64(s.phase != DONE) == 0ull)
            break;
        if (wall_clock64() - t0 > P.clock_limit) {
            // give up: the unfinished games keep finished = 0 (cleared before the launch)
            if (s.phase != DONE)
                __hip_atomic_store(&P.ctl[CTL_GAVE_UP], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            break;
        }

        bool moved = false, turn_over = false;
        if (s.phase == TURN) {
            if (legal_of(g_own, g_opp, SA) != 0ull && !g_over) {
                empties = 64 - __popcll(g_own | g_opp);
                search_begin(s, g_own, g_opp, R.window());
            } else {
                turn_over = true; // a pass, or no turn
            }
        }
        if (!search_step(s, K, lane, empties, R, SA)) {
            atomicOr(&P.ctl[CTL_OVERFLOW], 1u);
            s.phase = CLAIM;
            continue;
        }
        if (search_done(s)) {
            moved = true;
            turn_over = true;
        }
        if (turn_over) {
            const int64_t row = (int64_t)turn * P.stride + g;
            P.rec_own[row] = g_own;
            P.rec_opp[row] = g_opp;
            P.rec_valid[row] = moved ? 3 : 0;
            P.rec_move[row] = (int8_t)(moved ? s.root_move : -1);
            P.rec_score[row] = (int8_t)(moved ? s.v : 0);
            if constexpr (Rules::ROOT != LOWEST)
                P.rec_best[row] = moved ? s.best_set : 0ull;
            // the stone and the swap of sides
            const uint64_t f = moved ? flips_of(g_own, g_opp, (uint32_t)s.root_move) | (1ull << s.root_move) : 0ull;
            const uint64_t nown = g_opp & ~f;
            g_opp = g_own | f;
            g_own = nown;
            // the books
            const bool was_over = g_over;
            stones += moved ? 1 : 0;
            const bool passing = !moved && !was_over;
            if (passing && pass_flg)
                stones = 64;                 // a pass after a pass ends the game
            if (!was_over)
                pass_flg = passing;
            if (turn % 2 == 1)               // `while stone_num < 64` once per pair of turns
                g_over = was_over || stones >= 64;
            turn++;
            if (turn >= P.max_turns || (turn % 2 == 0 && g_over)) {
                P.turn[g] = turn;
                P.own[g] = g_own;
                P.opp[g] = g_opp;
                P.finished[g] = 1;
                s.phase = CLAIM;
            } else {
                s.phase = TURN;
            }
        }
    }
}

__global__ __launch_bounds__(WAVE) void play_endgame_kernel(PlayParams P)
{
    extern __shared__ __align__(16) unsigned char stack_lds[];
    play_endgame_games<SolverRules>(P, stack_lds);
}

struct PlayMovesParams : PlayParams {
    uint64_t *rec_best;
};

__global__ __launch_bounds__(WAVE) void play_endgame_moves_kernel(PlayMovesParams P)
{
    extern __shared__ __align__(16) unsigned char stack_lds[];
    play_endgame_games<SolverRulesT<BEST>>(P, stack_lds);
}

// a frame is pushed by a node with >= 2 empties: levels 0 .. max_empties - 2
int stack_levels(int max_empties) { return max_empties > 2 ? max_empties - 1 : 1; }

// the kernel's params from iago_play_endgame's arguments
void fill_play_params(PlayParams &P, const iago_play_endgame_args *a)
{
    P.own = a->own;
    P.opp = a->opp;
    P.turn = a->turn;
    P.stones = a->stones;
    P.pass_flg = a->pass_flg;
    P.parked = a->parked;
    P.n = a->n;
    P.stride = a->stride;
    P.rec_own = a->rec_own;
    P.rec_opp = a->rec_opp;
    P.rec_valid = a->rec_valid;
    P.rec_move = a->rec_move;
    P.rec_score = a->rec_score;
    P.finished = a->finished;
    P.ctl = a->ctl;
    P.max_turns = a->max_turns;
    P.max_empties = a->max_empties;
    P.levels = stack_levels(a->max_empties);
    P.clock_limit = (long long)a->time_limit_ms * 100000ll; // wall_clock64: 100 MHz
}

} // namespace

extern "C" int iago_solve_endgame(const iago_endgame_args *a, void *stream)
{
    const char *who = "iago_solve_endgame";
    if (!a)
        return iago_fail(IAGO_ERR_INVALID, "iago_solve_endgame: null args");
    if (a->n < 0 || (a->n > 0 && (!a->own || !a->opp || !a->score || !a->move || !a->nodes || !a->solved)) ||
        !a->ctl)
        return iago_fail(IAGO_ERR_INVALID, "iago_solve_endgame: null pointer or negative n");
    if (a->mode != IAGO_ENDGAME_EXACT && a->mode != IAGO_ENDGAME_WLD)
        return iago_fail(IAGO_ERR_INVALID, "iago_solve_endgame: mode must be IAGO_ENDGAME_EXACT or IAGO_ENDGAME_WLD");
    if (a->max_empties < 0 || a->max_empties > IAGO_ENDGAME_MAX_EMPTIES)
        return iago_fail(IAGO_ERR_INVALID, "iago_solve_endgame: max_empties must be in [0, 20]");
    if (a->time_limit_ms <= 0 || a->time_limit_ms > IAGO_ENDGAME_MAX_TIME_MS)
        return iago_fail(IAGO_ERR_INVALID, "iago_solve_endgame: time_limit_ms must be in [1, 600000]");
    for (int i = 0; i < 4; i++)
        if (a->reserved[i] != 0 || a->reserved0 != 0)
            return iago_fail(IAGO_ERR_INVALID, "iago_solve_endgame: reserved fields must be 0");
    hipStream_t s = (hipStream_t)stream;
    int cus = 0;
    const int rc = iago_search_prepare(who, a->ctl, 4, a->solved, "solved", a->n, s, &cus);
    if (rc != IAGO_OK || cus == 0)
        return rc;

    EndgameParams P;
    P.own = a->own;
    P.opp = a->opp;
    P.n = a->n;
    P.score = a->score;
    P.move = a->move;
    P.nodes = a->nodes;
    P.solved = a->solved;
    P.ctl = a->ctl;
    P.wld = a->mode == IAGO_ENDGAME_WLD;
    P.max_empties = a->max_empties;
    P.levels = stack_levels(a->max_empties);
    P.clock_limit = (long long)a->time_limit_ms * 100000ll; // wall_clock64: 100 MHz
    iago_search_launch((const void *)endgame_kernel, &P, P.levels, Stack<SolverRules>::FRAME_BYTES, a->n, cus, s);
    return iago_check_launch(who);
}

extern "C" int iago_play_endgame(const iago_play_endgame_args *a, void *stream)
{
    const char *who = "iago_play_endgame";
    if (!a)
        return iago_fail(IAGO_ERR_INVALID, "iago_play_endgame: null args");
    if (a->n < 0 || !a->ctl ||
        (a->n > 0 && (!a->own || !a->opp || !a->turn || !a->stones || !a->pass_flg || !a->parked || !a->rec_own ||
                      !a->rec_opp || !a->rec_valid || !a->rec_move || !a->rec_score || !a->finished)))
        return iago_fail(IAGO_ERR_INVALID, "iago_play_endgame: null pointer or negative n");
    if (a->stride < a->n)
        return iago_fail(IAGO_ERR_INVALID, "iago_play_endgame: stride >= n expected");
    if (a->max_turns < 1 || a->max_turns > IAGO_MAX_TURNS)
        return iago_fail(IAGO_ERR_INVALID, "iago_play_endgame: max_turns must be in [1, IAGO_MAX_TURNS]");
    if (a->max_empties < 0 || a->max_empties > IAGO_ENDGAME_MAX_EMPTIES)
        return iago_fail(IAGO_ERR_INVALID, "iago_play_endgame: max_empties must be in [0, 20]");
    if (a->time_limit_ms <= 0 || a->time_limit_ms > IAGO_ENDGAME_MAX_TIME_MS)
        return iago_fail(IAGO_ERR_INVALID, "iago_play_endgame: time_limit_ms must be in [1, 600000]");
    for (int i = 0; i < 4; i++)
        if (a->reserved[i] != 0 || a->reserved0 != 0)
            return iago_fail(IAGO_ERR_INVALID, "iago_play_endgame: reserved fields must be 0");
    hipStream_t s = (hipStream_t)stream;
    int cus = 0;
    const int rc = iago_search_prepare(who, a->ctl, 4, a->finished, "finished", a->n, s, &cus);
    if (rc != IAGO_OK || cus == 0)
        return rc;

    PlayParams P;
    fill_play_params(P, a);
    iago_search_launch((const void *)play_endgame_kernel, &P, P.levels, Stack<SolverRules>::FRAME_BYTES, a->n, cus, s);
    return iago_check_launch(who);
}

extern "C" int iago_solve_endgame_moves(const iago_endgame_moves_args *a, void *stream)
{
    const char *who = "iago_solve_endgame_moves";
    if (!a)
        return iago_fail(IAGO_ERR_INVALID, "iago_solve_endgame_moves: null args");
    if (a->n < 0 ||
        (a->n > 0 && (!a->own || !a->opp || !a->score || !a->move || !a->nodes || !a->solved || !a->best)) || !a->ctl)
        return iago_fail(IAGO_ERR_INVALID, "iago_solve_endgame_moves: null pointer or negative n");
    if (a->mode != IAGO_ENDGAME_EXACT && a->mode != IAGO_ENDGAME_WLD)
        return iago_fail(IAGO_ERR_INVALID,
                         "iago_solve_endgame_moves: mode must be IAGO_ENDGAME_EXACT or IAGO_ENDGAME_WLD");
    if (a->moves != IAGO_ENDGAME_MOVES_BEST && a->moves != IAGO_ENDGAME_MOVES_ALL)
        return iago_fail(IAGO_ERR_INVALID,
                         "iago_solve_endgame_moves: moves must be IAGO_ENDGAME_MOVES_BEST or IAGO_ENDGAME_MOVES_ALL");
    const bool all = a->moves == IAGO_ENDGAME_MOVES_ALL;
    if (!all && a->move_score)
        return iago_fail(IAGO_ERR_INVALID, "iago_solve_endgame_moves: move_score must be NULL under IAGO_ENDGAME_MOVES_BEST");
    if (all && a->n > 0 && !a->move_score)
        return iago_fail(IAGO_ERR_INVALID, "iago_solve_endgame_moves: move_score is required under IAGO_ENDGAME_MOVES_ALL");
    if (a->max_empties < 0 || a->max_empties > IAGO_ENDGAME_MAX_EMPTIES)
        return iago_fail(IAGO_ERR_INVALID, "iago_solve_endgame_moves: max_empties must be in [0, 20]");
    if (a->time_limit_ms <= 0 || a->time_limit_ms > IAGO_ENDGAME_MAX_TIME_MS)
        return iago_fail(IAGO_ERR_INVALID, "iago_solve_endgame_moves: time_limit_ms must be in [1, 600000]");
    for (int i = 0; i < 4; i++)
        if (a->reserved[i] != 0)
            return iago_fail(IAGO_ERR_INVALID, "iago_solve_endgame_moves: reserved fields must be 0");
    hipStream_t s = (hipStream_t)stream;
    int cus = 0;
    const int rc = iago_search_prepare(who, a->ctl, 4, a->solved, "solved", a->n, s, &cus);
    if (rc != IAGO_OK || cus == 0)
        return rc;
    // every cell starts as "no move": the search writes the legal moves of the roots it admits
    if (all && hipMemsetAsync(a->move_score, IAGO_ENDGAME_NO_MOVE & 0xFF, (size_t)a->n * 64, s) != hipSuccess) {
        (void)hipGetLastError();
        return iago_fail(IAGO_ERR_HIP, "iago_solve_endgame_moves: clearing move_score");
    }

    MovesParams P;
    P.own = a->own;
    P.opp = a->opp;
    P.n = a->n;
    P.score = a->score;
    P.move = a->move;
    P.nodes = a->nodes;
    P.solved = a->solved;
    P.ctl = a->ctl;
    P.wld = a->mode == IAGO_ENDGAME_WLD;
    P.max_empties = a->max_empties;
    P.levels = stack_levels(a->max_empties);
    P.clock_limit = (long long)a->time_limit_ms * 100000ll; // wall_clock64: 100 MHz
    P.best = a->best;
    P.move_score = a->move_score;
    const void *kernel = all ? (const void *)endgame_moves_kernel<ALL> : (const void *)endgame_moves_kernel<BEST>;
    iago_search_launch(kernel, &P, P.levels, Stack<SolverRules>::FRAME_BYTES, a->n, cus, s);
    return iago_check_launch(who);
}

extern "C" int iago_solve_endgame_split(const iago_endgame_split_args *a, void *stream)
{
    const char *who = "iago_solve_endgame_split";
    if (!a)
        return iago_fail(IAGO_ERR_INVALID, "iago_solve_endgame_split: null args");
    if (a->n < 0 || a->n > INT32_MAX || (a->n > 0 && (!a->own || !a->opp || !a->job_count || !a->job_first)) || !a->ctl)
        return iago_fail(IAGO_ERR_INVALID, "iago_solve_endgame_split: null pointer, negative n or n above 2^31 - 1");
    if (a->mode != IAGO_ENDGAME_EXACT && a->mode != IAGO_ENDGAME_WLD)
        return iago_fail(IAGO_ERR_INVALID,
                         "iago_solve_endgame_split: mode must be IAGO_ENDGAME_EXACT or IAGO_ENDGAME_WLD");
    if (a->split < 1 || a->split > IAGO_ENDGAME_MAX_SPLIT)
        return iago_fail(IAGO_ERR_INVALID, "iago_solve_endgame_split: split must be 1 or 2");
    if (a->max_empties < 0 || a->max_empties > IAGO_ENDGAME_MAX_EMPTIES)
        return iago_fail(IAGO_ERR_INVALID, "iago_solve_endgame_split: max_empties must be in [0, 20]");
    if (a->time_limit_ms <= 0 || a->time_limit_ms > IAGO_ENDGAME_MAX_TIME_MS)
        return iago_fail(IAGO_ERR_INVALID, "iago_solve_endgame_split: time_limit_ms must be in [1, 600000]");
    if (a->job_capacity < 0 || a->job_capacity > INT32_MAX)
        return iago_fail(IAGO_ERR_INVALID, "iago_solve_endgame_split: job_capacity must be in [0, 2^31 - 1]");
    const int job_arrays = (a->job_own != nullptr) + (a->job_opp != nullptr) + (a->job_root != nullptr) +
                           (a->job_path != nullptr) + (a->job_score != nullptr) + (a->job_move != nullptr) +
                           (a->job_nodes != nullptr) + (a->job_done != nullptr);
    if ((job_arrays != 0 && job_arrays != 8) || (job_arrays == 0 && a->job_capacity != 0))
        return iago_fail(IAGO_ERR_INVALID, "iago_solve_endgame_split: the job arrays are all given, or all null with "
                                           "job_capacity 0 (the count-only form)");
    const bool count_only = job_arrays == 0;
    if (!count_only && a->n > 0 && (!a->score || !a->move || !a->nodes || !a->solved))
        return iago_fail(IAGO_ERR_INVALID, "iago_solve_endgame_split: null score, move, nodes or solved");
    for (int i = 0; i < 4; i++)
        if (a->reserved[i] != 0)
            return iago_fail(IAGO_ERR_INVALID, "iago_solve_endgame_split: reserved fields must be 0");
    static_assert(IAGO_ENDGAME_SPLIT_CTL_WORDS == SPLIT_CTL_WORDS && IAGO_ENDGAME_MAX_SPLIT == MAX_SPLIT, "lane_split.hpp");
    hipStream_t s = (hipStream_t)stream;
    int cus = 0;
    const int rc = iago_search_prepare(who, a->ctl, IAGO_ENDGAME_SPLIT_CTL_WORDS, count_only ? nullptr : a->solved,
                                       "solved", a->n, s, &cus);
    if (rc != IAGO_OK || cus == 0)
        return rc;
    // every cell starts as "no move": the reduction writes the legal moves of the roots it answers
    if (!count_only && a->move_score &&
        hipMemsetAsync(a->move_score, IAGO_ENDGAME_NO_MOVE & 0xFF, (size_t)a->n * 64, s) != hipSuccess) {
        (void)hipGetLastError();
        return iago_fail(IAGO_ERR_HIP, "iago_solve_endgame_split: clearing move_score");
    }

    // 1. expand: count, sum, write
    split_expand(split_params_of(a, EmptiesJobs{a->max_empties}), count_only, s);
    if (count_only)
        return iago_check_launch(who);

    // 2. search: the lanes of iago_solve_endgame over the jobs
    EndgameJobParams J;
    J.own = a->job_own;
    J.opp = a->job_opp;
    J.score = a->job_score;
    J.move = a->job_move;
    J.nodes = a->job_nodes;
    J.done = a->job_done;
    J.ctl = a->ctl;
    J.wld = a->mode == IAGO_ENDGAME_WLD;
    J.levels = stack_levels(a->max_empties); // the deepest job is a root that must pass: max_empties empties
    J.clock_limit = (long long)a->time_limit_ms * 100000ll; // wall_clock64: 100 MHz
    iago_search_launch((const void *)endgame_jobs_kernel, &J, J.levels, Stack<SolverRules>::FRAME_BYTES,
                       a->job_capacity, cus, s);

    // 3. reduce
    ReduceParams<EmptiesJobs> R = reduce_params_of<EmptiesJobs>(a, a->solved);
    R.best = a->best;
    R.move_score = a->move_score;
    split_reduce(R, s);
    return iago_check_launch(who);
}

extern "C" int iago_play_endgame_moves(const iago_play_endgame_moves_args *m, void *stream)
{
    const char *who = "iago_play_endgame_moves";
    if (!m)
        return iago_fail(IAGO_ERR_INVALID, "iago_play_endgame_moves: null args");
    const iago_play_endgame_args *a = &m->play;
    if (a->n < 0 || !a->ctl ||
        (a->n > 0 && (!a->own || !a->opp || !a->turn || !a->stones || !a->pass_flg || !a->parked || !a->rec_own ||
                      !a->rec_opp || !a->rec_valid || !a->rec_move || !a->rec_score || !a->finished || !m->rec_best)))
        return iago_fail(IAGO_ERR_INVALID, "iago_play_endgame_moves: null pointer or negative n");
    if (a->stride < a->n)
        return iago_fail(IAGO_ERR_INVALID, "iago_play_endgame_moves: stride >= n expected");
    if (a->max_turns < 1 || a->max_turns > IAGO_MAX_TURNS)
        return iago_fail(IAGO_ERR_INVALID, "iago_play_endgame_moves: max_turns must be in [1, IAGO_MAX_TURNS]");
    if (a->max_empties < 0 || a->max_empties > IAGO_ENDGAME_MAX_EMPTIES)
        return iago_fail(IAGO_ERR_INVALID, "iago_play_endgame_moves: max_empties must be in [0, 20]");
    if (a->time_limit_ms <= 0 || a->time_limit_ms > IAGO_ENDGAME_MAX_TIME_MS)
        return iago_fail(IAGO_ERR_INVALID, "iago_play_endgame_moves: time_limit_ms must be in [1, 600000]");
    for (int i = 0; i < 4; i++)
        if (a->reserved[i] != 0 || a->reserved0 != 0 || m->reserved[i] != 0)
            return iago_fail(IAGO_ERR_INVALID, "iago_play_endgame_moves: reserved fields must be 0");
    hipStream_t s = (hipStream_t)stream;
    int cus = 0;
    const int rc = iago_search_prepare(who, a->ctl, 4, a->finished, "finished", a->n, s, &cus);
    if (rc != IAGO_OK || cus == 0)
        return rc;

    PlayMovesParams P;
    fill_play_params(P, a);
    P.rec_best = m->rec_best;
    iago_search_launch((const void *)play_endgame_moves_kernel, &P, P.levels, Stack<SolverRules>::FRAME_BYTES, a->n, cus,
                       s);
    return iago_check_launch(who);
}
