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
// What the entry points share with alphabeta_kernel.hip's -- the refusals, the range checks, the params' base, the
// launches -- is lane_host.hpp's.
#include "abi_common.hpp"
#include "lane_host.hpp"
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

struct EndgameParams : LaneParams<int8_t> {
    int64_t n;
    int32_t wld;
    int32_t max_empties;

    __device__ __forceinline__ bool admit(int64_t pos, uint64_t &o, uint64_t &p, int &empties) const
    {
        o = own[pos];
        p = opp[pos];
        empties = 64 - __popcll(o | p);
        return ((o & p) == 0ull && empties <= max_empties) || refuse(pos);
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
        LaneParams::finish(pos, s);
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
struct EndgameJobParams : LaneParams<int8_t> {
    int32_t wld;

    __device__ __forceinline__ bool admit(int64_t pos, uint64_t &o, uint64_t &p, int &empties) const
    {
        o = own[pos];
        p = opp[pos];
        empties = 64 - __popcll(o | p); // (at most the root's, which is at most max_empties)
        return true;
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

constexpr int FRAME_BYTES = Stack<SolverRules>::FRAME_BYTES; // (the root's rule does not change the frame)

// a frame is pushed by a node with >= 2 empties: levels 0 .. max_empties - 2
int stack_levels(int max_empties) { return max_empties > 2 ? max_empties - 1 : 1; }

// the root kernels' params from the arguments of iago_solve_endgame and iago_solve_endgame_moves
template <class Args>
void fill_endgame_params(EndgameParams &P, const Args *a)
{
    fill_lane_params(P, a->own, a->opp, a->score, a->move, a->nodes, a->solved, a->ctl, stack_levels(a->max_empties),
                     a->time_limit_ms);
    P.n = a->n;
    P.wld = a->mode == IAGO_ENDGAME_WLD;
    P.max_empties = a->max_empties;
}

// Both play entry points: the checks, the clears and the launch.  m: iago_play_endgame_moves' arguments around a, or null
int play_endgame(const char *who, const iago_play_endgame_args *a, const iago_play_endgame_moves_args *m, hipStream_t s)
{
    if (a->n < 0 || !a->ctl ||
        (a->n > 0 && (!a->own || !a->opp || !a->turn || !a->stones || !a->pass_flg || !a->parked || !a->rec_own ||
                      !a->rec_opp || !a->rec_valid || !a->rec_move || !a->rec_score || !a->finished ||
                      (m && !m->rec_best))))
        return refuse(who, "null pointer or negative n");
    if (a->stride < a->n)
        return refuse(who, "stride >= n expected");
    if (a->max_turns < 1 || a->max_turns > IAGO_MAX_TURNS)
        return refuse(who, "max_turns must be in [1, IAGO_MAX_TURNS]");
    if (const int rc = check_max_empties(who, a->max_empties))
        return rc;
    if (const int rc = check_time_limit(who, a->time_limit_ms))
        return rc;
    if (const int rc = check_reserved(who, a->reserved, a->reserved0))
        return rc;
    if (m)
        if (const int rc = check_reserved(who, m->reserved))
            return rc;

    PlayMovesParams P;
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
    P.clock_limit = clock_limit_of(a->time_limit_ms);
    P.rec_best = m ? m->rec_best : nullptr;
    if (m)
        return lane_run(who, P, a->finished, "finished", a->n, nullptr, (const void *)play_endgame_moves_kernel,
                        FRAME_BYTES, s);
    return lane_run(who, static_cast<PlayParams &>(P), a->finished, "finished", a->n, nullptr,
                    (const void *)play_endgame_kernel, FRAME_BYTES, s);
}

} // namespace

extern "C" int iago_solve_endgame(const iago_endgame_args *a, void *stream)
{
    const char *who = "iago_solve_endgame";
    if (!a)
        return refuse(who, "null args");
    if (const int rc = check_roots(who, a, a->solved))
        return rc;
    if (const int rc = check_mode(who, a->mode))
        return rc;
    if (const int rc = check_max_empties(who, a->max_empties))
        return rc;
    if (const int rc = check_time_limit(who, a->time_limit_ms))
        return rc;
    if (const int rc = check_reserved(who, a->reserved, a->reserved0))
        return rc;

    EndgameParams P;
    fill_endgame_params(P, a);
    return lane_run(who, P, a->solved, "solved", a->n, nullptr, (const void *)endgame_kernel, FRAME_BYTES,
                    (hipStream_t)stream);
}

extern "C" int iago_solve_endgame_moves(const iago_endgame_moves_args *a, void *stream)
{
    const char *who = "iago_solve_endgame_moves";
    if (!a)
        return refuse(who, "null args");
    if (const int rc = check_roots(who, a, a->solved, a->best != nullptr))
        return rc;
    if (const int rc = check_mode(who, a->mode))
        return rc;
    if (a->moves != IAGO_ENDGAME_MOVES_BEST && a->moves != IAGO_ENDGAME_MOVES_ALL)
        return refuse(who, "moves must be IAGO_ENDGAME_MOVES_BEST or IAGO_ENDGAME_MOVES_ALL");
    const bool all = a->moves == IAGO_ENDGAME_MOVES_ALL;
    if (!all && a->move_score)
        return refuse(who, "move_score must be NULL under IAGO_ENDGAME_MOVES_BEST");
    if (all && a->n > 0 && !a->move_score)
        return refuse(who, "move_score is required under IAGO_ENDGAME_MOVES_ALL");
    if (const int rc = check_max_empties(who, a->max_empties))
        return rc;
    if (const int rc = check_time_limit(who, a->time_limit_ms))
        return rc;
    if (const int rc = check_reserved(who, a->reserved))
        return rc;

    MovesParams P;
    fill_endgame_params(P, a);
    P.best = a->best;
    P.move_score = a->move_score;
    const void *kernel = all ? (const void *)endgame_moves_kernel<ALL> : (const void *)endgame_moves_kernel<BEST>;
    return lane_run(who, P, a->solved, "solved", a->n, a->move_score, kernel, FRAME_BYTES, (hipStream_t)stream);
}

extern "C" int iago_solve_endgame_split(const iago_endgame_split_args *a, void *stream)
{
    const char *who = "iago_solve_endgame_split";
    if (!a)
        return refuse(who, "null args");
    if (const int rc = split_check_roots(who, a))
        return rc;
    if (const int rc = check_mode(who, a->mode))
        return rc;
    if (a->split < 1 || a->split > IAGO_ENDGAME_MAX_SPLIT)
        return refuse(who, "split must be 1 or 2");
    if (const int rc = check_max_empties(who, a->max_empties))
        return rc;
    if (const int rc = check_time_limit(who, a->time_limit_ms))
        return rc;
    bool count_only = false;
    if (const int rc = split_check_jobs(who, a, a->solved, "solved", &count_only))
        return rc;
    if (const int rc = check_reserved(who, a->reserved))
        return rc;
    static_assert(IAGO_ENDGAME_SPLIT_CTL_WORDS == SPLIT_CTL_WORDS && IAGO_ENDGAME_MAX_SPLIT == MAX_SPLIT, "lane_split.hpp");

    EndgameJobParams J;
    J.wld = a->mode == IAGO_ENDGAME_WLD;
    return split_run(who, a, count_only, a->solved, "solved", EmptiesJobs{a->max_empties},
                     (const void *)endgame_jobs_kernel, J, stack_levels(a->max_empties), FRAME_BYTES, (hipStream_t)stream);
}

extern "C" int iago_play_endgame(const iago_play_endgame_args *a, void *stream)
{
    const char *who = "iago_play_endgame";
    return a ? play_endgame(who, a, nullptr, (hipStream_t)stream) : refuse(who, "null args");
}

extern "C" int iago_play_endgame_moves(const iago_play_endgame_moves_args *m, void *stream)
{
    const char *who = "iago_play_endgame_moves";
    return m ? play_endgame(who, &m->play, m, (hipStream_t)stream) : refuse(who, "null args");
}
