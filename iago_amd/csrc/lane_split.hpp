// lane_split.hpp -- the device-side ROOT SPLIT that the fixed-depth opponent (iago_alphabeta_moves_split,
// alphabeta_kernel.hip) and the exact endgame solver (iago_solve_endgame_split, endgame_kernel.hip) share: every root's
// first one or two plies are expanded into JOBS, lane_search.hpp's search runs a lane per job, and a thread per root
// takes the jobs' values back.  Every stage is a launch of its own on the caller's stream: a stage reads what the one
// before it wrote.
//   1. split_count_kernel (a thread per root: job_count), split_scan_kernel (ONE workgroup: job_first = the exclusive
//      sum, the total into ctl[4] / [5], ctl[6] when it exceeds the capacity), split_write_kernel (a thread per root:
//      its jobs in canonical order -- first move ascending, then second move -- from job_first on);
//   2. the search's own jobs kernel: the job count claimed from ctl with split_jobs_to_claim();
//   3. split_reduce_kernel (a thread per root): its run of jobs minimaxed back, the sign turned once per ply.
// A node is a job when no split ply is left or its mover has no legal move (a root or a child that must pass, a
// finished game), else it is expanded.  What differs between the two searches comes as a KIND struct (an object: it
// carries the launch's depth or max_empties):
//   Score                      the type of a value in memory (int16 the opponent, int8 the solver)
//   NEG_INF                    below every value
//   MOVES                      the reduction also answers the set of the best moves and every first move's value
//   admits(own, opp)           false: the root is refused (counted in ctl[2], no job, its done flag stays 0)
//   left(own, opp, plies)      a job's "depth left", path[0]: what its lane searches it with
#pragma once
#include "lane_search.hpp"

namespace iago {
namespace lane {

// a split launch's further ctl words
constexpr int CTL_JOBS_LO = 4;
constexpr int CTL_JOBS_HI = 5;
constexpr int CTL_JOB_OVERFLOW = 6;
constexpr int SPLIT_CTL_WORDS = 8;
constexpr int MAX_SPLIT = 2;

constexpr int SPLIT_BLOCK = 256;
constexpr int SCAN_BLOCK = 1024;

// the jobs a wave of a jobs kernel may claim: their number as the scan left it, none after an overflow of the arrays
__device__ __forceinline__ int64_t split_jobs_to_claim(const uint32_t *ctl)
{
    return ctl[CTL_JOB_OVERFLOW] != 0u ? 0 : (int64_t)ctl[CTL_JOBS_LO];
}

// The job record: position, root, path = (depth left, first move, second move, 0; -1 for a move the path lacks)
template <class Kind>
struct SplitParams {
    const uint64_t *own;
    const uint64_t *opp;
    int64_t n;
    int32_t split;
    Kind kind;
    int32_t *job_count;
    int64_t *job_first;
    int64_t capacity;
    uint64_t *job_own;
    uint64_t *job_opp;
    int32_t *job_root;
    int8_t *job_path;
    uint8_t *job_done;
    uint32_t *ctl;
};

// The jobs of root i in canonical order (first move ascending, then second move): counted, and with WRITE written from
// job_first[i] on.  A node is a job when no split ply is left or its mover has no legal move, else it is expanded.
template <bool WRITE, class Kind>
__device__ __forceinline__ int expand_root(const SplitParams<Kind> &P, int64_t i, uint64_t own, uint64_t opp,
                                           const ShiftAmounts &SA)
{
    int64_t at = 0;
    if constexpr (WRITE)
        at = P.job_first[i];
    int count = 0;
    auto job = [&](uint64_t o, uint64_t p, int plies, int m1, int m2) {
        if constexpr (WRITE) {
            const int64_t j = at + count;
            if (j < P.capacity) { // (always: the total fits or nothing is written)
                P.job_own[j] = o;
                P.job_opp[j] = p;
                P.job_root[j] = (int32_t)i;
                P.job_path[4 * j + 0] = (int8_t)P.kind.left(o, p, plies);
                P.job_path[4 * j + 1] = (int8_t)m1;
                P.job_path[4 * j + 2] = (int8_t)m2;
                P.job_path[4 * j + 3] = 0;
                P.job_done[j] = 0;
            }
        }
        count++;
    };
    uint64_t legal = legal_of(own, opp, SA);
    if (legal == 0ull) {
        job(own, opp, 0, -1, -1); // a root that must pass, or a finished game
        return count;
    }
    while (legal) {
        const uint32_t m1 = lowest_bit(legal);
        legal &= legal - 1ull;
        const uint64_t f = flips_of(own, opp, m1);
        const uint64_t cown = opp & ~f, copp = own | f | (1ull << m1);
        uint64_t replies = P.split >= 2 ? legal_of(cown, copp, SA) : 0ull;
        if (replies == 0ull) {
            job(cown, copp, 1, (int)m1, -1); // the last split ply, or a child that cannot move
            continue;
        }
        while (replies) {
            const uint32_t m2 = lowest_bit(replies);
            replies &= replies - 1ull;
            const uint64_t g = flips_of(cown, copp, m2);
            job(copp & ~g, cown | g | (1ull << m2), 2, (int)m1, (int)m2);
        }
    }
    return count;
}

template <class Kind>
__global__ __launch_bounds__(SPLIT_BLOCK) void split_count_kernel(SplitParams<Kind> P)
{
    const int64_t i = (int64_t)blockIdx.x * SPLIT_BLOCK + threadIdx.x;
    if (i >= P.n)
        return;
    const ShiftAmounts SA = opaque_shift_amounts();
    const uint64_t own = P.own[i], opp = P.opp[i];
    int count = 0;
    if (!P.kind.admits(own, opp))
        atomicAdd(&P.ctl[CTL_REFUSED], 1u); // refused: no job, done stays 0
    else
        count = expand_root<false>(P, i, own, opp, SA);
    P.job_count[i] = count;
}

// job_first = the exclusive sum of job_count, the total into ctl: ONE workgroup, SCAN_BLOCK roots per round.
// capacity < 0: the count-only form, which has no overflow.  (Kind: a name of its own per search, nothing else.)
template <class Kind>
__global__ __launch_bounds__(SCAN_BLOCK) void split_scan_kernel(const int32_t *count, int64_t *first, int64_t n,
                                                                int64_t capacity, uint32_t *ctl)
{
    __shared__ long long wave_sum[SCAN_BLOCK / WAVE];
    const int lane = threadIdx.x % WAVE, w = threadIdx.x / WAVE;
    long long carry = 0;
    for (int64_t base = 0; base < n; base += SCAN_BLOCK) {
        const int64_t i = base + threadIdx.x;
        const long long c = i < n ? count[i] : 0;
        long long x = c;
        for (int o = 1; o < WAVE; o <<= 1) {
            const long long y = __shfl_up(x, o);
            if (lane >= o)
                x += y;
        }
        if (lane == WAVE - 1)
            wave_sum[w] = x;
        __syncthreads();
        long long before = 0, total = 0;
        for (int k = 0; k < SCAN_BLOCK / WAVE; k++) {
            const long long v = wave_sum[k];
            before += k < w ? v : 0;
            total += v;
        }
        if (i < n)
            first[i] = carry + before + x - c;
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        ctl[CTL_JOBS_LO] = (uint32_t)carry;
        ctl[CTL_JOBS_HI] = (uint32_t)((unsigned long long)carry >> 32);
        if (capacity >= 0 && carry > capacity)
            ctl[CTL_JOB_OVERFLOW] = 1u;
    }
}

template <class Kind>
__global__ __launch_bounds__(SPLIT_BLOCK) void split_write_kernel(SplitParams<Kind> P)
{
    const int64_t i = (int64_t)blockIdx.x * SPLIT_BLOCK + threadIdx.x;
    if (i >= P.n || P.ctl[CTL_JOB_OVERFLOW] != 0u || P.job_count[i] == 0)
        return;
    const ShiftAmounts SA = opaque_shift_amounts();
    expand_root<true>(P, i, P.own[i], P.opp[i], SA);
}

template <class Kind>
struct ReduceParams {
    using Score = typename Kind::Score;
    int64_t n;
    const int32_t *job_count;
    const int64_t *job_first;
    const int8_t *job_path;
    const Score *job_score;
    const int8_t *job_move;
    const int64_t *job_nodes;
    const uint8_t *job_done;
    Score *score;
    int8_t *move;
    int64_t *nodes;
    uint8_t *done;
    uint64_t *best;      // Kind::MOVES, may be null: the set of the first moves reaching the score
    int8_t *move_score;  // Kind::MOVES, may be null: [n][64], every first move's value (the caller filled the rest)
    const uint32_t *ctl;
};

// A thread per root: its run of jobs minimaxed back, the sign turned once per ply of the path; the first maximum in
// canonical order is the lowest-indexed move of the best value.  nodes: 1 for the root, 1 per expanded child and the
// jobs' own; a root that is its own job counts only the job's.
template <class Kind>
__global__ __launch_bounds__(SPLIT_BLOCK) void split_reduce_kernel(ReduceParams<Kind> P)
{
    using Score = typename Kind::Score;
    const int64_t i = (int64_t)blockIdx.x * SPLIT_BLOCK + threadIdx.x;
    if (i >= P.n || P.ctl[CTL_JOB_OVERFLOW] != 0u)
        return;
    const int count = P.job_count[i];
    if (count == 0) { // refused: done stays 0
        P.score[i] = 0;
        P.move[i] = 0;
        P.nodes[i] = 0;
        if constexpr (Kind::MOVES) {
            if (P.best)
                P.best[i] = 0ull;
        }
        return;
    }
    const int64_t j0 = P.job_first[i];
    bool all = true;
    for (int64_t j = j0; j < j0 + count; j++)
        all = all && P.job_done[j] != 0;
    if (!all) // (a give-up: the unfinished jobs hold nothing, the root is not written)
        return;
    int best = Kind::NEG_INF, best_m = -1;
    uint64_t best_set = 0ull;
    // the value v of the first move m, from the root's mover's view
    auto take = [&](int m, int v) {
        if constexpr (Kind::MOVES) {
            if (P.move_score)
                P.move_score[64 * i + m] = (int8_t)v;
            if (v > best)
                best_set = 1ull << m;
            else if (v == best)
                best_set |= 1ull << m;
        }
        if (v > best) {
            best = v;
            best_m = m;
        }
    };
    int child_m = -1, child_best = Kind::NEG_INF; // the expanded child whose jobs are being taken back
    int64_t nodes = 1;
    for (int64_t j = j0; j < j0 + count; j++) {
        nodes += P.job_nodes[j];
        const int m1 = P.job_path[4 * j + 1], m2 = P.job_path[4 * j + 2];
        const int v = P.job_score[j];
        if (m1 < 0) { // the root is the job
            best = v;
            best_m = P.job_move[j];
            nodes--;
            continue;
        }
        if (m1 != child_m && child_m >= 0) {
            take(child_m, -child_best);
            child_m = -1;
        }
        if (m2 < 0) { // the child is the job
            take(m1, -v);
        } else {
            if (child_m < 0) {
                child_m = m1;
                child_best = Kind::NEG_INF;
                nodes++;
            }
            child_best = max(child_best, -v);
        }
    }
    if (child_m >= 0)
        take(child_m, -child_best);
    P.score[i] = (Score)best;
    P.move[i] = (int8_t)best_m;
    P.nodes[i] = nodes;
    if constexpr (Kind::MOVES) {
        if (P.best)
            P.best[i] = best_set;
    }
    P.done[i] = 1;
}

// The pointers of the C structs' job arrays as the stages read them, for both searches' launch code
template <class Kind, class Args>
SplitParams<Kind> split_params_of(const Args *a, const Kind &kind)
{
    SplitParams<Kind> E;
    E.own = a->own;
    E.opp = a->opp;
    E.n = a->n;
    E.split = a->split;
    E.kind = kind;
    E.job_count = a->job_count;
    E.job_first = a->job_first;
    E.capacity = a->job_capacity;
    E.job_own = a->job_own;
    E.job_opp = a->job_opp;
    E.job_root = a->job_root;
    E.job_path = a->job_path;
    E.job_done = a->job_done;
    E.ctl = a->ctl;
    return E;
}

template <class Kind, class Args>
ReduceParams<Kind> reduce_params_of(const Args *a, uint8_t *done)
{
    ReduceParams<Kind> R;
    R.n = a->n;
    R.job_count = a->job_count;
    R.job_first = a->job_first;
    R.job_path = a->job_path;
    R.job_score = a->job_score;
    R.job_move = a->job_move;
    R.job_nodes = a->job_nodes;
    R.job_done = a->job_done;
    R.score = a->score;
    R.move = a->move;
    R.nodes = a->nodes;
    R.done = done;
    R.best = nullptr;
    R.move_score = nullptr;
    if constexpr (Kind::MOVES) {
        R.best = a->best;
        R.move_score = a->move_score;
    }
    R.ctl = a->ctl;
    return R;
}

// stage 1 on stream s: count, scan, and unless count_only write
template <class Kind>
void split_expand(const SplitParams<Kind> &E, bool count_only, hipStream_t s)
{
    const unsigned roots_grid = (unsigned)((E.n + SPLIT_BLOCK - 1) / SPLIT_BLOCK);
    hipLaunchKernelGGL(split_count_kernel<Kind>, dim3(roots_grid), dim3(SPLIT_BLOCK), 0, s, E);
    hipLaunchKernelGGL(split_scan_kernel<Kind>, dim3(1), dim3(SCAN_BLOCK), 0, s, (const int32_t *)E.job_count,
                       E.job_first, E.n, count_only ? (int64_t)-1 : E.capacity, E.ctl);
    if (!count_only)
        hipLaunchKernelGGL(split_write_kernel<Kind>, dim3(roots_grid), dim3(SPLIT_BLOCK), 0, s, E);
}

// stage 3 on stream s
template <class Kind>
void split_reduce(const ReduceParams<Kind> &R, hipStream_t s)
{
    const unsigned roots_grid = (unsigned)((R.n + SPLIT_BLOCK - 1) / SPLIT_BLOCK);
    hipLaunchKernelGGL(split_reduce_kernel<Kind>, dim3(roots_grid), dim3(SPLIT_BLOCK), 0, s, R);
}

} // namespace lane
} // namespace iago
