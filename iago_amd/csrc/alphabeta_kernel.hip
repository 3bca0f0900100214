// alphabeta_kernel.hip -- iago_alphabeta_moves: a fixed-depth alpha-beta search on a hand-written evaluation, batched;
// iago_random_moves: the random opening draw of a match against it.
//
// Contract: include/iago_hip_serving.h.  The rule, in integers:
//   search(own, opp, d): no legal move -> neither side has one: terminal(own, opp), at any depth; else
//   -search(opp, own, d), a pass in place that costs no depth.  d == 0 -> eval(own, opp).  Else the maximum over the
//   legal moves m of -search(play(own, opp, m), d - 1).
//   terminal = 10000 sign(D) + 100 D, D = #own - #opp; eval = the seven square classes below + 8 x the mobility difference.
// The search is lane_search.hpp's, the one of endgame_kernel.hip -- a lane per position, the node in registers, an
// explicit stack in LDS, passes in place, positions claimed from ctl, the root's tie rule -- on YardstickRules below:
//   * a node's remaining levels are the depth left, not its empties: a node of remaining depth 1 pushes no frame -- each
//     of its children is a LEAF, evaluated in the parent in one step (eval is antisymmetric, so a leaf whose mover must
//     pass needs no second look: its value is eval or, when neither side can move, terminal);
//   * values are int16 (|eval| < 10000 <= |terminal| <= 16400 unless the game is drawn), the window is +-32767, a frame
//     is 32 B per level and lane (alpha / beta / best as int16);
//   * move order below the root's tie rule: a corner first, then at nodes of remaining depth >= ORDER_DEPTH the move
//     with the fewest replies (ties: lowest index), else index order.  Only `nodes` depends on it.
// iago_alphabeta_moves_split spreads every root over many lanes: the first one or two plies are expanded into JOBS
// (position, depth left) on the device, the same search runs a lane per job (alphabeta_jobs_kernel: the job count read
// from ctl, every lane's depth from its job), and a thread per root takes the values back.  Every job has the full window,
// so its value and its node count are those of iago_alphabeta_moves on that position, whatever else runs beside it.
// The expansion, the scan, the job record and the reduction are lane_split.hpp's, shared with iago_solve_endgame_split;
// the entry points' refusals, range checks, params' base and launches are lane_host.hpp's, shared with the solver's.
#include "abi_common.hpp"
#include "lane_host.hpp"
#include "lane_search.hpp"
#include "lane_split.hpp"
#include "othello_dev.hpp"

#include "../../include/iago_hip_serving.h"

using namespace iago;
using namespace iago::lane;

namespace {

constexpr int ORDER_DEPTH = 3;     // nodes with at least this much depth left try their moves fewest replies first
constexpr uint32_t OPEN_KEY = IAGO_OPENING_KEY;
constexpr uint64_t CORNERS = 0x8100000000000081ull;

template <int V>
__device__ __forceinline__ int class_term(uint64_t own, uint64_t opp, uint64_t mask)
{
    return V * (__popcll(own & mask) - __popcll(opp & mask));
}

// the static evaluation from the mover's view; lo / lp: the mover's and the other side's legal moves
__device__ __forceinline__ int eval_value(uint64_t own, uint64_t opp, uint64_t lo, uint64_t lp)
{
    return class_term<100>(own, opp, 0x8100000000000081ull) + class_term<-20>(own, opp, 0x4281000000008142ull) +
           class_term<-50>(own, opp, 0x0042000000004200ull) + class_term<10>(own, opp, 0x2400810000810024ull) +
           class_term<5>(own, opp, 0x1800008181000018ull) + class_term<-2>(own, opp, 0x003C424242423C00ull) +
           class_term<-1>(own, opp, 0x00003C3C3C3C0000ull) + 8 * (__popcll(lo) - __popcll(lp));
}

struct YardstickRules {
    static constexpr RootRule ROOT = LOWEST;
    using Info = uint64_t;
    static constexpr int NEG_INF = -32768;
    static constexpr bool COUNT_LAST = false;
    static constexpr bool LEAF_CHILDREN = true;

    __device__ __forceinline__ int window() const { return 32767; }

    __device__ __forceinline__ int terminal(uint64_t own, uint64_t opp) const
    {
        const int d = __popcll(own) - __popcll(opp); // empty squares go to nobody (judge)
        return 10000 * ((d > 0) - (d < 0)) + 100 * d;
    }

    // search(own, opp, 0): terminal when neither side can move, else eval (a mover that must pass: -eval(opp, own) = eval)
    __device__ __forceinline__ int leaf(uint64_t own, uint64_t opp, const ShiftAmounts &SA) const
    {
        const uint64_t lo = legal_of(own, opp, SA), lp = legal_of(opp, own, SA);
        return (lo | lp) == 0ull ? terminal(own, opp) : eval_value(own, opp, lo, lp);
    }

    // a corner, else (depth left >= ORDER_DEPTH) the fewest opponent replies, else the lowest index
    __device__ __forceinline__ uint32_t pick_move(uint64_t own, uint64_t opp, uint64_t moves, int rem,
                                                  const ShiftAmounts &SA) const
    {
        const uint64_t corners = moves & CORNERS;
        if (corners != 0ull)
            return lowest_bit(corners);
        return rem >= ORDER_DEPTH ? fewest_replies(own, opp, moves, SA) : lowest_bit(moves);
    }

    // alpha, beta, best as int16 (offset 32768), pass flag, move tried
    static __device__ __forceinline__ Info pack(int alpha, int beta, int best, uint32_t passed, uint32_t m)
    {
        const uint32_t lo = (uint32_t)(alpha + 32768) | ((uint32_t)(beta + 32768) << 16);
        const uint32_t hi = (uint32_t)(best + 32768) | (passed << 16) | (m << 17);
        return ((uint64_t)hi << 32) | lo;
    }

    static __device__ __forceinline__ int unpack(Info info, Search &s)
    {
        const uint32_t lo = (uint32_t)info, hi = (uint32_t)(info >> 32);
        s.alpha = (int)(lo & 0xFFFFu) - 32768;
        s.beta = (int)(lo >> 16) - 32768;
        s.best = (int)(hi & 0xFFFFu) - 32768;
        s.passed = (hi >> 16) & 1u;
        return (int)(hi >> 17);
    }
};

struct AlphaBetaParams : LaneParams<int16_t> {
    int64_t n;
    int32_t depth;

    __device__ __forceinline__ bool admit(int64_t pos, uint64_t &o, uint64_t &p, int &) const
    {
        o = own[pos];
        p = opp[pos];
        return (o & p) == 0ull || refuse(pos);
    }
};

// The jobs of iago_alphabeta_moves_split as the search reads and answers them: positions with a depth of their own
struct JobParams : LaneParams<int16_t> {
    const int8_t *path;      // [jobs][4]: depth left, first move, second move, 0

    __device__ __forceinline__ bool admit(int64_t pos, uint64_t &o, uint64_t &p, int &depth) const
    {
        o = own[pos];
        p = opp[pos];
        depth = path[4 * pos];
        return true;
    }
};

__global__ __launch_bounds__(WAVE) void alphabeta_kernel(AlphaBetaParams P)
{
    extern __shared__ __align__(16) unsigned char stack_lds[];
    search_wave(P, YardstickRules{}, P.n, P.depth, stack_lds);
}

// over the jobs of a split search: their number read from ctl (none after an overflow of the job arrays)
__global__ __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(8, 8))) void alphabeta_jobs_kernel(JobParams P)
{
    extern __shared__ __align__(16) unsigned char stack_lds[];
    const int64_t n = split_jobs_to_claim(P.ctl);
    if ((int64_t)blockIdx.x * WAVE >= n) // nothing to claim: the wave leaves at once
        return;
    search_wave(P, YardstickRules{}, n, 0, stack_lds);
}

// ---- iago_alphabeta_moves_split: the stages of lane_split.hpp on the opponent's KIND -- a job's depth left is the
// launch's depth minus the plies of its path, values are int16, the reduction answers score and move alone.
struct DepthJobs {
    using Score = int16_t;
    static constexpr int NEG_INF = YardstickRules::NEG_INF;
    static constexpr bool MOVES = false;
    int32_t depth;

    __device__ __forceinline__ bool admits(uint64_t own, uint64_t opp) const { return (own & opp) == 0ull; }
    __device__ __forceinline__ int left(uint64_t, uint64_t, int plies) const { return depth - plies; }
};

// ---- iago_random_moves: the opening draw, a thread per game

__global__ __launch_bounds__(256) void random_moves_kernel(const uint64_t *own, const uint64_t *opp, int64_t n,
                                                           uint32_t key0, uint32_t key1, uint32_t id_base,
                                                           uint32_t id_mod, uint32_t turn, int8_t *move)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n)
        return;
    const ShiftAmounts SA = opaque_shift_amounts();
    uint64_t legal = legal_of(own[g], opp[g], SA);
    const uint32_t K = (uint32_t)__popcll(legal);
    int m = -1;
    if (K != 0u) {
        uint32_t c[4] = {id_base + (uint32_t)(g % (int64_t)id_mod), turn >> 2, 0u, 0u};
        philox4x32_10(c, key0, key1 ^ OPEN_KEY);
        const uint32_t lo = (turn & 1u) ? c[1] : c[0], hi = (turn & 1u) ? c[3] : c[2]; // (selects: no indexed array)
        const uint32_t w = (turn & 2u) ? hi : lo;
        const uint32_t r = __umulhi(w, K); // (uint64(w) * K) >> 32, below K
        for (uint32_t i = 0; i < r; i++)
            legal &= legal - 1ull;
        m = (int)lowest_bit(legal);
    }
    move[g] = (int8_t)m;
}

constexpr int FRAME_BYTES = Stack<YardstickRules>::FRAME_BYTES;

} // namespace

extern "C" int iago_alphabeta_moves(const iago_alphabeta_args *a, void *stream)
{
    const char *who = "iago_alphabeta_moves";
    if (!a)
        return refuse(who, "null args");
    if (const int rc = check_roots(who, a, a->done))
        return rc;
    if (a->depth < 1 || a->depth > IAGO_ALPHABETA_MAX_DEPTH)
        return refuse(who, "depth must be in [1, 10]");
    if (const int rc = check_time_limit(who, a->time_limit_ms))
        return rc;
    if (const int rc = check_reserved(who, a->reserved))
        return rc;

    AlphaBetaParams P;
    // a frame is pushed by a node with >= 2 levels below it: levels 0 .. depth - 2
    fill_lane_params(P, a->own, a->opp, a->score, a->move, a->nodes, a->done, a->ctl, a->depth, a->time_limit_ms);
    P.n = a->n;
    P.depth = a->depth;
    return lane_run(who, P, a->done, "done", a->n, nullptr, (const void *)alphabeta_kernel, FRAME_BYTES,
                    (hipStream_t)stream);
}

extern "C" int iago_alphabeta_moves_split(const iago_alphabeta_split_args *a, void *stream)
{
    const char *who = "iago_alphabeta_moves_split";
    if (!a)
        return refuse(who, "null args");
    if (const int rc = split_check_roots(who, a))
        return rc;
    if (a->depth < 2 || a->depth > IAGO_ALPHABETA_MAX_DEPTH)
        return refuse(who, "depth must be in [2, 10]");
    if (a->split < 1 || a->split > IAGO_ALPHABETA_MAX_SPLIT || a->split >= a->depth)
        return refuse(who, "split must be 1 or 2 and below depth");
    if (const int rc = check_time_limit(who, a->time_limit_ms))
        return rc;
    bool count_only = false;
    if (const int rc = split_check_jobs(who, a, a->done, "done", &count_only))
        return rc;
    if (const int rc = check_reserved(who, a->reserved, a->reserved0))
        return rc;
    static_assert(IAGO_ALPHABETA_SPLIT_CTL_WORDS == SPLIT_CTL_WORDS && IAGO_ALPHABETA_MAX_SPLIT == MAX_SPLIT,
                  "lane_split.hpp");

    JobParams J;
    J.path = a->job_path;
    return split_run(who, a, count_only, a->done, "done", DepthJobs{a->depth}, (const void *)alphabeta_jobs_kernel, J,
                     a->depth, FRAME_BYTES, (hipStream_t)stream);
}

extern "C" int iago_random_moves(const uint64_t *own, const uint64_t *opp, int64_t n, uint64_t seed, uint32_t id_base,
                                 uint32_t id_mod, int32_t turn, int8_t *move, void *stream)
{
    if (n < 0 || (n > 0 && (!own || !opp || !move)))
        return iago_fail(IAGO_ERR_INVALID, "iago_random_moves: null pointer or negative n");
    if (id_mod == 0u)
        return iago_fail(IAGO_ERR_INVALID, "iago_random_moves: id_mod >= 1 expected");
    if (turn < 0 || turn >= IAGO_MAX_TURNS)
        return iago_fail(IAGO_ERR_INVALID, "iago_random_moves: turn must be in [0, IAGO_MAX_TURNS)");
    if (n == 0)
        return IAGO_OK;
    const unsigned grid = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(random_moves_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, own, opp, n, (uint32_t)seed,
                       (uint32_t)(seed >> 32), id_base, id_mod, (uint32_t)turn, move);
    return iago_check_launch("iago_random_moves");
}
