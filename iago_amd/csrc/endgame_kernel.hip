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
#include "abi_common.hpp"
#include "othello_dev.hpp"
#include "othello_lane.hpp"

#include "../../include/iago_hip_serving.h"

#include <atomic>

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

enum Phase : uint32_t { CLAIM = 0, ENTER = 1, NEXT = 2, RETURN = 3, DONE = 4 };

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

__device__ __forceinline__ uint64_t legal_of(uint64_t own, uint64_t opp, const ShiftAmounts &SA)
{
    return legal_moves_1(own, opp, rev64(own), rev64(opp), SA);
}

__device__ __forceinline__ uint64_t flips_of(uint64_t own, uint64_t opp, uint32_t m)
{
    return flips_1(own, opp, rev64(own), rev64(opp), m);
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

__global__ __launch_bounds__(WAVE) void endgame_kernel(EndgameParams P)
{
    extern __shared__ __align__(16) unsigned char stack_lds[];
    const uint32_t lane = threadIdx.x;
    const int levels = P.levels;
    uint64_t *st_own = (uint64_t *)stack_lds;
    uint64_t *st_opp = st_own + levels * WAVE;
    uint64_t *st_moves = st_opp + levels * WAVE;
    uint32_t *st_info = (uint32_t *)(st_moves + levels * WAVE);

    const ShiftAmounts SA = opaque_shift_amounts();
    const long long t0 = wall_clock64();
    const int root_alpha = P.wld ? -1 : -65, root_beta = P.wld ? 1 : 65;

    uint32_t phase = CLAIM;
    int64_t pos = 0;
    uint64_t own = 0ull, opp = 0ull, moves = 0ull;
    int alpha = 0, beta = 0, best = 0, v = 0;
    int d = 0, empties0 = 0;
    uint32_t passed = 0u;
    int root_move = -1;
    int64_t nodes = 0;

    while (true) {
        if (phase == CLAIM) {
            if (__hip_atomic_load(&P.ctl[CTL_GAVE_UP], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {
                phase = DONE;
            } else {
                pos = (int64_t)atomicAdd(&P.ctl[CTL_CLAIM], 1u);
                if (pos >= P.n) {
                    phase = DONE;
                } else {
                    own = P.own[pos];
                    opp = P.opp[pos];
                    empties0 = 64 - __popcll(own | opp);
                    if ((own & opp) != 0ull || empties0 > P.max_empties) {
                        // refused: solved stays 0
                        atomicAdd(&P.ctl[CTL_REFUSED], 1u);
                        P.score[pos] = 0;
                        P.move[pos] = 0;
                        P.nodes[pos] = 0;
                    } else {
                        d = 0;
                        alpha = root_alpha;
                        beta = root_beta;
                        nodes = 0;
                        root_move = -1;
                        phase = ENTER;
                    }
                }
            }
        }
        if (__builtin_amdgcn_ballot_w64(phase != DONE) == 0ull)
            break;
        if (wall_clock64() - t0 > P.clock_limit) {
            // give up: the unfinished positions keep solved = 0 (cleared before the launch)
            if (phase != DONE)
                __hip_atomic_store(&P.ctl[CTL_GAVE_UP], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            break;
        }

        if (phase == ENTER) {
            nodes++;
            passed = 0u;
            const int e = empties0 - d;
            uint64_t legal = legal_of(own, opp, SA);
            if (legal == 0ull) {
                const uint64_t other = legal_of(opp, own, SA);
                if (other == 0ull) { // neither side can move: the game is over
                    v = final_score(own, opp, P.wld);
                    if (d == 0)
                        root_move = -2;
                    phase = RETURN;
                } else { // pass in place
                    const uint64_t t = own;
                    own = opp;
                    opp = t;
                    const int a = alpha;
                    alpha = -beta;
                    beta = -a;
                    passed = 1u;
                    legal = other;
                }
            }
            if (phase == ENTER) {
                if (e == 1) { // the last empty: its move ends the game
                    const uint32_t m = lowest_bit(legal);
                    const uint64_t f = flips_of(own, opp, m);
                    nodes++;
                    v = final_score(own | f | (1ull << m), opp & ~f, P.wld);
                    if (passed)
                        v = -v;
                    if (d == 0)
                        root_move = passed ? -1 : (int)m;
                    phase = RETURN;
                } else {
                    moves = legal;
                    best = NEG_INF;
                    if (d == 0)
                        root_move = passed ? -1 : 64; // 64: no move yet (above every index)
                    phase = NEXT;
                }
            }
        } else if (phase == RETURN && d > 0) {
            // the child's value, back in the parent
            d--;
            const int k = d * WAVE + (int)lane;
            own = st_own[k];
            opp = st_opp[k];
            moves = st_moves[k];
            const uint32_t info = st_info[k];
            alpha = (int)(info & 0xFFu) - 128;
            beta = (int)((info >> 8) & 0xFFu) - 128;
            best = (int)((info >> 16) & 0xFFu) - 128;
            passed = (info >> 24) & 1u;
            const int m = (int)(info >> 25);
            v = -v;
            if (d == 0 && !passed) {
                // root: the lowest index among the moves of the best value (the window kept every tie exact)
                if (v > best || (v == best && m < root_move)) {
                    best = v;
                    root_move = m;
                }
            } else {
                best = max(best, v);
                alpha = max(alpha, best);
                if (alpha >= beta)
                    moves = 0ull; // cut-off
            }
            phase = NEXT;
        }

        if (phase == NEXT) {
            const bool root = d == 0 && !passed;
            uint32_t m = 0u;
            int a_child = alpha;
            bool go = false;
            while (moves != 0ull) {
                m = pick_move(own, opp, moves, empties0 - d, SA);
                moves &= ~(1ull << m);
                if (root && best > NEG_INF) // a tie of a lower index must come back exact, a higher one must beat best
                    a_child = max(alpha, (int)m < root_move ? best - 1 : best);
                if (a_child < beta) {
                    go = true;
                    break;
                }
            }
            if (go) {
                if (d >= P.levels) { // cannot happen for an admitted position (d <= empties - 2): never write past it
                    atomicOr(&P.ctl[CTL_OVERFLOW], 1u);
                    phase = CLAIM;
                    continue;
                }
                const int k = d * WAVE + (int)lane;
                st_own[k] = own;
                st_opp[k] = opp;
                st_moves[k] = moves;
                st_info[k] = pack_info(alpha, beta, best, passed, m);
                const uint64_t f = flips_of(own, opp, m);
                const uint64_t nown = opp & ~f;
                opp = own | f | (1ull << m);
                own = nown;
                const int a = a_child;
                alpha = -beta;
                beta = -a;
                d++;
                phase = ENTER;
            } else {
                v = passed ? -best : best;
                phase = RETURN;
            }
        }

        if (phase == RETURN && d == 0) {
            P.score[pos] = (int8_t)v;
            P.move[pos] = (int8_t)root_move;
            P.nodes[pos] = nodes;
            P.solved[pos] = 1;
            phase = CLAIM;
        }
    }
}

std::atomic<int> g_cus{0};

int device_cus()
{
    int c = g_cus.load(std::memory_order_relaxed);
    if (c > 0)
        return c;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) !=
                                                 hipSuccess || c <= 0) {
        (void)hipGetLastError();
        return 0;
    }
    g_cus.store(c, std::memory_order_relaxed);
    return c;
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
    const int cus = device_cus();
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
