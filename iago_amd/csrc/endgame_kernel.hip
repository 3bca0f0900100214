// endgame_kernel.hip -- iago_solve_endgame: the exact value of Othello positions with few empties, batched.
//
// Contract: include/iago_hip_serving.h.  One LANE PER POSITION runs a negamax alpha-beta depth-first search on the
// rules of othello_lane.hpp with an explicit stack:
//   * the node a lane works on lives in registers (own, opp, the untried moves, alpha, beta, the best value so far);
//     descending pushes it as one FRAME onto the lane's stack in LDS, laid out [level][lane] (28 B per level: own,
//     opp, untried moves, a packed word of alpha / beta / best / pass flag / move tried), returning pops it.  No
//     runtime-indexed register array anywhere: the kernel has no scratch.
//   * a pass pushes no frame: the node swaps the sides and negates the window in place and negates its value when
//     it returns, so a lane never holds more frames than the position had empties;
//   * one step of the loop is one node entered or one child's value taken back; lanes that finish a position claim
//     the next one from a counter in ctl, so a wave is not held back by its one deep position;
//   * move order: at nodes with more than ORDER_EMPTIES empties the untried move with the fewest replies for the
//     opponent goes first (fastest first; ties: lowest index), below that index order; a node with one empty is
//     counted directly (the board is full after its move);
//   * the root alone differs: every move that could tie the best value with a lower index is searched with a window
//     that keeps that tie exact, so `move` is the lowest-indexed move reaching the value, whatever the order;
//   * mode WLD scores the end of the game by its sign: the same search on values in {-1, 0, 1}, window (-1, 1)
//     around 0 at the root.
// Every lane reads the wall clock once per step: past time_limit_ms the launch gives up (ctl[0] = 1), every position
// it has not finished keeps solved = 0.
// The search of one position is the device function solve_step below; iago_play_endgame (play_endgame_kernel: one lane per
// GAME) calls the same function once per turn of a game and plays the moves, to the game's end.
#include "abi_common.hpp"
#include "othello_dev.hpp"
#include "othello_lane.hpp"

#include "../../include/iago_hip_serving.h"

using namespace iago;
using namespace iago::lane;

namespace {

constexpr int WAVE = 64;          // one wave per workgroup: the stack is the wave's own
constexpr int ORDER_EMPTIES = 6;  // nodes with more empties than this try their moves fastest first
constexpr int NEG_INF = -100;     // below every score (scores are in [-64, 64])
constexpr int FRAME_BYTES = 28;   // per level and lane: own, opp, moves (u64), info (u32)

// ctl words (uint32): what the header documents, and the claim counter
constexpr int CTL_GAVE_UP = 0;
constexpr int CTL_CLAIM = 1;
constexpr int CTL_REFUSED = 2;
constexpr int CTL_OVERFLOW = 3;

enum Phase : uint32_t { CLAIM = 0, ENTER = 1, NEXT = 2, RETURN = 3, DONE = 4, TURN = 5 };

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
};

// alpha, beta, best in 8 bits each (offset 128), pass flag, move tried
__device__ __forceinline__ uint32_t pack_info(int alpha, int beta, int best, uint32_t passed, uint32_t m)
{
    return (uint32_t)(alpha + 128) | ((uint32_t)(beta + 128) << 8) | ((uint32_t)(best + 128) << 16) |
           (passed << 24) | (m << 25);
}

__device__ __forceinline__ int final_score(uint64_t own, uint64_t opp, int32_t wld)
{
    const int d = __popcll(own) - __popcll(opp); // empty squares go to nobody (judge)
    return wld ? (d > 0) - (d < 0) : d;
}

// The untried move to search next: fewest opponent replies first above ORDER_EMPTIES empties, else the lowest index.
__device__ __forceinline__ uint32_t pick_move(uint64_t own, uint64_t opp, uint64_t moves, int empties,
                                              const ShiftAmounts &SA)
{
    uint32_t best_m = lowest_bit(moves);
    if (empties > ORDER_EMPTIES) {
        uint32_t best_mob = 65u;
        uint64_t rem = moves;
        while (rem) {
            const uint32_t m = lowest_bit(rem);
            rem &= rem - 1ull;
            const uint64_t f = flips_of(own, opp, m);
            const uint32_t mob = (uint32_t)__popcll(legal_of(opp & ~f, own | f | (1ull << m), SA));
            if (mob < best_mob) {
                best_mob = mob;
                best_m = m;
            }
        }
    }
    return best_m;
}

// ---- the search of ONE position as a state machine in the lane's registers, shared by the two kernels below

// a lane's search: the node it works on, the value on its way back, the depth, the root's books
struct Solve {
    uint32_t phase;
    uint64_t own, opp, moves;
    int alpha, beta, best, v;
    int d, empties0;
    uint32_t passed;
    int root_move;
    int64_t nodes;
};

// the wave's stack in LDS, [level][lane]
struct Stack {
    uint64_t *own, *opp, *moves;
    uint32_t *info;
    int levels;
};

__device__ __forceinline__ Stack make_stack(unsigned char *lds, int levels)
{
    Stack K;
    K.own = (uint64_t *)lds;
    K.opp = K.own + levels * WAVE;
    K.moves = K.opp + levels * WAVE;
    K.info = (uint32_t *)(K.moves + levels * WAVE);
    K.levels = levels;
    return K;
}

// the root of a new search: (own, opp) with own to move, the full window
__device__ __forceinline__ void solve_begin(Solve &s, uint64_t own, uint64_t opp, int empties0, int32_t wld)
{
    s.own = own;
    s.opp = opp;
    s.empties0 = empties0;
    s.d = 0;
    s.alpha = wld ? -1 : -65;
    s.beta = wld ? 1 : 65;
    s.nodes = 0;
    s.root_move = -1;
    s.phase = ENTER;
}

// the search is over: v is the root's value, root_move its move
__device__ __forceinline__ bool solve_done(const Solve &s) { return s.phase == RETURN && s.d == 0; }

// One step of a lane that is searching (phase ENTER, NEXT or RETURN below the root; any other phase: nothing): one node
// entered or one child's value taken back.  false: the stack would overflow (cannot happen for a position with at most
// levels + 1 empties) -- nothing was written past it, the caller drops the position.
__device__ __forceinline__ bool solve_step(Solve &s, const Stack &K, uint32_t lane, int32_t wld, const ShiftAmounts &SA)
{
    if (s.phase == ENTER) {
        s.nodes++;
        s.passed = 0u;
        const int e = s.empties0 - s.d;
        uint64_t legal = legal_of(s.own, s.opp, SA);
        if (legal == 0ull) {
            const uint64_t other = legal_of(s.opp, s.own, SA);
            if (other == 0ull) { // neither side can move: the game is over
                s.v = final_score(s.own, s.opp, wld);
                if (s.d == 0)
                    s.root_move = -2;
                s.phase = RETURN;
            } else { // pass in place
                const uint64_t t = s.own;
                s.own = s.opp;
                s.opp = t;
                const int a = s.alpha;
                s.alpha = -s.beta;
                s.beta = -a;
                s.passed = 1u;
                legal = other;
            }
        }
        if (s.phase == ENTER) {
            if (e == 1) { // the last empty: its move ends the game
                const uint32_t m = lowest_bit(legal);
                const uint64_t f = flips_of(s.own, s.opp, m);
                s.nodes++;
                s.v = final_score(s.own | f | (1ull << m), s.opp & ~f, wld);
                if (s.passed)
                    s.v = -s.v;
                if (s.d == 0)
                    s.root_move = s.passed ? -1 : (int)m;
                s.phase = RETURN;
            } else {
                s.moves = legal;
                s.best = NEG_INF;
                if (s.d == 0)
                    s.root_move = s.passed ? -1 : 64; // 64: no move yet (above every index)
                s.phase = NEXT;
            }
        }
    } else if (s.phase == RETURN && s.d > 0) {
        // the child's value, back in the parent
        s.d--;
        const int k = s.d * WAVE + (int)lane;
        s.own = K.own[k];
        s.opp = K.opp[k];
        s.moves = K.moves[k];
        const uint32_t info = K.info[k];
        s.alpha = (int)(info & 0xFFu) - 128;
        s.beta = (int)((info >> 8) & 0xFFu) - 128;
        s.best = (int)((info >> 16) & 0xFFu) - 128;
        s.passed = (info >> 24) & 1u;
        const int m = (int)(info >> 25);
        s.v = -s.v;
        if (s.d == 0 && !s.passed) {
            // root: the lowest index among the moves of the best value (the window kept every tie exact)
            if (s.v > s.best || (s.v == s.best && m < s.root_move)) {
                s.best = s.v;
                s.root_move = m;
            }
        } else {
            s.best = max(s.best, s.v);
            s.alpha = max(s.alpha, s.best);
            if (s.alpha >= s.beta)
                s.moves = 0ull; // cut-off
        }
        s.phase = NEXT;
    }

    if (s.phase == NEXT) {
        const bool root = s.d == 0 && !s.passed;
        uint32_t m = 0u;
        int a_child = s.alpha;
        bool go = false;
        while (s.moves != 0ull) {
            m = pick_move(s.own, s.opp, s.moves, s.empties0 - s.d, SA);
            s.moves &= ~(1ull << m);
            if (root && s.best > NEG_INF) // a tie of a lower index must come back exact, a higher one must beat best
                a_child = max(s.alpha, (int)m < s.root_move ? s.best - 1 : s.best);
            if (a_child < s.beta) {
                go = true;
                break;
            }
        }
        if (go) {
            if (s.d >= K.levels) // cannot happen for an admitted position (d <= empties - 2): never write past it
                return false;
            const int k = s.d * WAVE + (int)lane;
            K.own[k] = s.own;
            K.opp[k] = s.opp;
            K.moves[k] = s.moves;
            K.info[k] = pack_info(s.alpha, s.beta, s.best, s.passed, m);
            const uint64_t f = flips_of(s.own, s.opp, m);
            const uint64_t nown = s.opp & ~f;
            s.opp = s.own | f | (1ull << m);
            s.own = nown;
            const int a = a_child;
            s.alpha = -s.beta;
            s.beta = -a;
            s.d++;
            s.phase = ENTER;
        } else {
            s.v = s.passed ? -s.best : s.best;
            s.phase = RETURN;
        }
    }
    return true;
}

__global__ __launch_bounds__(WAVE) void endgame_kernel(EndgameParams P)
{
    extern __shared__ __align__(16) unsigned char stack_lds[];
    const uint32_t lane = threadIdx.x;
    const Stack K = make_stack(stack_lds, P.levels);
    const ShiftAmounts SA = opaque_shift_amounts();
    const long long t0 = wall_clock64();

    Solve s = {};
    s.phase = CLAIM;
    int64_t pos = 0;

    while (true) {
        if (s.phase == CLAIM) {
            if (__hip_atomic_load(&P.ctl[CTL_GAVE_UP], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {
                s.phase = DONE;
            } else {
                pos = (int64_t)atomicAdd(&P.ctl[CTL_CLAIM], 1u);
                if (pos >= P.n) {
                    s.phase = DONE;
                } else {
                    const uint64_t own = P.own[pos], opp = P.opp[pos];
                    const int empties0 = 64 - __popcll(own | opp);
                    if ((own & opp) != 0ull || empties0 > P.max_empties) {
                        // refused: solved stays 0
                        atomicAdd(&P.ctl[CTL_REFUSED], 1u);
                        P.score[pos] = 0;
                        P.move[pos] = 0;
                        P.nodes[pos] = 0;
                    } else {
                        solve_begin(s, own, opp, empties0, P.wld);
                    }
                }
            }
        }
        if (__builtin_amdgcn_ballot_w64(s.phase != DONE) == 0ull)
            break;
        if (wall_clock64() - t0 > P.clock_limit) {
            // give up: the unfinished positions keep solved = 0 (cleared before the launch)
            if (s.phase != DONE)
                __hip_atomic_store(&P.ctl[CTL_GAVE_UP], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            break;
        }

        if (!solve_step(s, K, lane, P.wld, SA)) {
            atomicOr(&P.ctl[CTL_OVERFLOW], 1u);
            s.phase = CLAIM;
            continue;
        }

        if (solve_done(s)) {
            P.score[pos] = (int8_t)s.v;
            P.move[pos] = (int8_t)s.root_move;
            P.nodes[pos] = s.nodes;
            P.solved[pos] = 1;
            s.phase = CLAIM;
        }
    }
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

// One LANE PER GAME, claimed from the counter: at every turn the mover's position is solved with solve_step (EXACT) and
// the move is played with the books of the persistent search's play_move (game.py:117-142,253-255): a stone per move, a
// pass after a pass sets stones = 64, the end of the game is tested once per pair of turns.  TURN: at a turn's start.
__global__ __launch_bounds__(WAVE) void play_endgame_kernel(PlayParams P)
{
    extern __shared__ __align__(16) unsigned char stack_lds[];
    const uint32_t lane = threadIdx.x;
    const Stack K = make_stack(stack_lds, P.levels);
    const ShiftAmounts SA = opaque_shift_amounts();
    const long long t0 = wall_clock64();

    Solve s = {};
    s.phase = CLAIM;
    int64_t g = 0;
    uint64_t g_own = 0ull, g_opp = 0ull; // the game's position, own = the side to move
    int turn = 0, stones = 0;
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
            if (legal_of(g_own, g_opp, SA) != 0ull && !g_over)
                solve_begin(s, g_own, g_opp, 64 - __popcll(g_own | g_opp), 0);
            else
                turn_over = true; // a pass, or no turn
        }
        if (!solve_step(s, K, lane, 0, SA)) {
            atomicOr(&P.ctl[CTL_OVERFLOW], 1u);
            s.phase = CLAIM;
            continue;
        }
        if (solve_done(s)) {
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

} // namespace

extern "C" int iago_solve_endgame(const iago_endgame_args *a, void *stream)
{
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
    if (hipMemsetAsync(a->ctl, 0, 4 * sizeof(uint32_t), s) != hipSuccess) {
        (void)hipGetLastError();
        return iago_fail(IAGO_ERR_HIP, "iago_solve_endgame: clearing ctl");
    }
    if (a->n == 0)
        return IAGO_OK;
    if (hipMemsetAsync(a->solved, 0, (size_t)a->n, s) != hipSuccess) {
        (void)hipGetLastError();
        return iago_fail(IAGO_ERR_HIP, "iago_solve_endgame: clearing solved");
    }
    const int cus = iago_device_cus();
    if (cus <= 0)
        return iago_fail(IAGO_ERR_HIP, "iago_solve_endgame: no HIP device");

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
    // a frame is pushed by a node with >= 2 empties: levels 0 .. max_empties - 2
    P.levels = a->max_empties > 2 ? a->max_empties - 1 : 1;
    P.clock_limit = (long long)a->time_limit_ms * 100000ll; // wall_clock64: 100 MHz
    const int lds = P.levels * WAVE * FRAME_BYTES;
    // every workgroup resident at once (the give-up is per wave's own clock): at most what the CUs hold
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, endgame_kernel, WAVE, lds) != hipSuccess ||
        per_cu <= 0) {
        (void)hipGetLastError();
        per_cu = 1;
    }
    const int64_t want = (a->n + WAVE - 1) / WAVE;
    const int64_t cap = (int64_t)cus * per_cu;
    const unsigned grid = (unsigned)(want < cap ? want : cap);
    hipLaunchKernelGGL(endgame_kernel, dim3(grid), dim3(WAVE), lds, s, P);
    return iago_check_launch("iago_solve_endgame");
}

extern "C" int iago_play_endgame(const iago_play_endgame_args *a, void *stream)
{
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
    if (hipMemsetAsync(a->ctl, 0, 4 * sizeof(uint32_t), s) != hipSuccess) {
        (void)hipGetLastError();
        return iago_fail(IAGO_ERR_HIP, "iago_play_endgame: clearing ctl");
    }
    if (a->n == 0)
        return IAGO_OK;
    if (hipMemsetAsync(a->finished, 0, (size_t)a->n, s) != hipSuccess) {
        (void)hipGetLastError();
        return iago_fail(IAGO_ERR_HIP, "iago_play_endgame: clearing finished");
    }
    const int cus = iago_device_cus();
    if (cus <= 0)
        return iago_fail(IAGO_ERR_HIP, "iago_play_endgame: no HIP device");

    PlayParams P;
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
    P.levels = a->max_empties > 2 ? a->max_empties - 1 : 1;
    P.clock_limit = (long long)a->time_limit_ms * 100000ll; // wall_clock64: 100 MHz
    const int lds = P.levels * WAVE * FRAME_BYTES;
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, play_endgame_kernel, WAVE, lds) != hipSuccess ||
        per_cu <= 0) {
        (void)hipGetLastError();
        per_cu = 1;
    }
    const int64_t want = (a->n + WAVE - 1) / WAVE;
    const int64_t cap = (int64_t)cus * per_cu;
    const unsigned grid = (unsigned)(want < cap ? want : cap);
    hipLaunchKernelGGL(play_endgame_kernel, dim3(grid), dim3(WAVE), lds, s, P);
    return iago_check_launch("iago_play_endgame");
}
