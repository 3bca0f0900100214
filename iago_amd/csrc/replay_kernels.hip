// replay_kernels.hip -- a minibatch out of the replay window of self-play rows, every row in one of the board's eight
// symmetries (gfx950) + its C ABI.  Contract and the rule of the draw: include/iago_hip_training.h, iago_replay_sample.
#include "abi_common.hpp"
#include "board_sym_dev.hpp"
#include "othello_dev.hpp"

#include "../../include/iago_hip_training.h"

using namespace iago;

namespace {

constexpr int BLOCK = 256;            // 4 waves, one output row per wave and pass
constexpr int ROWS = BLOCK / 64;
constexpr unsigned MAX_GRID = 8192;   // (32 workgroups per CU's worth; more rows take further passes)
constexpr uint32_t REPLAY_KEY = 0x52504C59u; // ("RPLY"; EXPLORE_KEY and the match key are its siblings)

// One wave per output row, lane = destination cell: the visit row is gathered within the slot's 256 bytes and written
// whole; slot and variant are the same in every lane, so the boards, the move and z are computed uniformly and stored
// by lane 0.  No LDS, no barrier: a wave whose rows are done leaves.
__global__ __launch_bounds__(BLOCK) void replay_sample_kernel(const iago_replay_sample_args P)
{
    const int lane = threadIdx.x & 63;
    const uint32_t count = (uint32_t)P.count;
    const uint32_t key0 = (uint32_t)P.seed, key1 = (uint32_t)(P.seed >> 32) ^ REPLAY_KEY;
    const int64_t stride = (int64_t)gridDim.x * ROWS;
    for (int64_t j = (int64_t)blockIdx.x * ROWS + (threadIdx.x >> 6); j < P.n; j += stride) {
        int32_t slot;
        uint32_t sym;
        if (P.slot_in) {
            slot = P.slot_in[j];
            sym = P.sym_in[j];
        } else {
            uint32_t c[4] = {(uint32_t)j, P.step, 0u, 0u};
            philox4x32_10(c, key0, key1);
            slot = (int32_t)__umulhi(c[0], count); // (uint64(c[0]) * count) >> 32 < count < 2^31
            sym = c[1] & 7u;
        }
        slot = __builtin_amdgcn_readfirstlane(slot); // (the same in every lane: say so)
        sym = (uint32_t)__builtin_amdgcn_readfirstlane((int)sym);
        const bool ok = (uint32_t)slot < count && sym < 8u; // (a negative slot is a large unsigned one)
        uint64_t o = 0ull, p = 0ull;
        int mv = -1, zz = 0, visits = 0;
        if (ok) { // nothing is read for a row that fails the check
            const int k = (int)sym;
            visits = P.pi[(int64_t)slot * 64 + act_variant_inverse(lane, k)];
            o = bb_variant(P.own[slot], k);
            p = bb_variant(P.opp[slot], k);
            mv = act_variant((int)P.move[slot], k);
            zz = (int)P.z[slot];
        }
        P.pi_out[j * 64 + lane] = visits;
        if (lane != 0)
            continue;
        P.own_out[j] = o;
        P.opp_out[j] = p;
        P.move_out[j] = (int8_t)mv;
        P.z_out[j] = (int8_t)zz;
        if (P.result_out)
            P.result_out[j] = (float)zz;
        if (P.slot_out)
            P.slot_out[j] = slot;
        if (P.sym_out)
            P.sym_out[j] = (uint8_t)sym;
        if (!ok && P.flags)
            atomicOr(P.flags, 1u);
    }
}

// One thread per row: the eight variants walked once (bb_canonical).
__global__ __launch_bounds__(BLOCK) void canonical_rows_kernel(const uint64_t *__restrict__ own,
                                                                const uint64_t *__restrict__ opp, int64_t n,
                                                                uint64_t *__restrict__ c_own,
                                                                uint64_t *__restrict__ c_opp, uint8_t *__restrict__ sym)
{
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
        uint64_t o = own[i], p = opp[i];
        const int k = bb_canonical(o, p);
        c_own[i] = o;
        c_opp[i] = p;
        sym[i] = (uint8_t)k;
    }
}

constexpr int64_t I32_MAX = 0x7FFFFFFF, I32_MIN = -I32_MAX - 1;

__device__ __forceinline__ int64_t clamp_i32(int64_t x) { return x > I32_MAX ? I32_MAX : x < I32_MIN ? I32_MIN : x; }

// The sorted rows' group numbers, checked, into the groups' first rows: sorted row i opens group group[i] where that
// is one more than its predecessor's.  A numbering that does not start at 0 or steps by anything but 0 or 1 raises
// bit 0, and merge_count_kernel then leaves n_unique = 0: the reduction does nothing.
__global__ __launch_bounds__(BLOCK) void merge_heads_kernel(const iago_replay_merge_args P)
{
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < P.count; i += stride) {
        const int64_t g = P.group[i], prev = i ? (int64_t)P.group[i - 1] : -1;
        // (with prev >= -1 a passing g lies in 0 .. i, inside every [count] output)
        if (prev < -1 || (g != prev && g != prev + 1) || (i == 0 && g != 0))
            atomicOr(P.flags, (uint32_t)IAGO_REPLAY_MERGE_BAD_INPUT);
        else if (g != prev)
            P.first[g] = i;
    }
}
__global__ void merge_count_kernel(const iago_replay_merge_args P) // one thread, after merge_heads_kernel
{
    const int64_t last = P.group[P.count - 1];
    const bool ok = !(*P.flags & (uint32_t)IAGO_REPLAY_MERGE_BAD_INPUT) && last >= 0 && last < P.count;
    *P.n_unique = ok ? (int32_t)(last + 1) : 0;
}

constexpr int SPREAD = 512; // a group of more sorted rows than this is summed by several waves,
constexpr int CHUNK = 256;  // each over the part of it that lies in one chunk of this many sorted rows

struct Span {
    int64_t start, end;
};
// The sorted rows of group g.  first[] holds every group of a checked numbering; the clamps keep anything else from
// becoming an index.
__device__ __forceinline__ Span group_span(const iago_replay_merge_args &P, int64_t g, int64_t groups)
{
    const int64_t count = P.count;
    int64_t start = P.first[g], end = g + 1 < groups ? P.first[g + 1] : count;
    start = start < 0 ? 0 : start > count ? count : start;
    end = end < start ? start : end > count ? count : end;
    return Span{start, end};
}
// A group's boards are those of its first sorted row (zeros where that row's slot is out of range).
__device__ __forceinline__ void group_key(const iago_replay_merge_args &P, int64_t start, uint64_t &key_o, uint64_t &key_p)
{
    key_o = key_p = 0ull;
    if (start >= P.count)
        return;
    const int slot = P.order[start];
    if ((uint32_t)slot < (uint32_t)P.count) { // (count < 2^31: a negative slot is a large unsigned one)
        key_o = P.c_own[slot];
        key_p = P.c_opp[slot];
    }
}
// The sorted rows from .. to-1, all of the group with the boards key, into this lane's canonical cell (acc) and this
// lane's share of the results (z_acc).  A pass takes 64 rows: each lane loads one row's slot, canonical boards,
// variant and result, then the wave walks the rows with slot and variant out of the lanes' registers.  A row whose slot
// is out of range, whose variant is above 7 or whose canonical boards are not the group's is left out (bad).
__device__ __forceinline__ void sum_rows(const iago_replay_merge_args &P, int64_t from, int64_t to, uint64_t key_o,
                                         uint64_t key_p, uint64_t inverse, int lane, int64_t &acc, int &z_acc, bool &bad)
{
    for (int64_t base = from; base < to; base += 64) {
        const int m = to - base < 64 ? (int)(to - base) : 64;
        int my_slot = -1, my_sym = 0, my_z = 0;
        if (lane < m) {
            my_slot = P.order[base + lane];
            if ((uint32_t)my_slot < (uint32_t)P.count) {
                my_sym = P.sym[my_slot];
                my_z = P.z[my_slot];
                if (P.c_own[my_slot] != key_o || P.c_opp[my_slot] != key_p || my_sym > 7)
                    my_slot = -1;
            } else {
                my_slot = -1;
            }
            if (my_slot < 0) {
                bad = true;
                my_z = 0;
            }
        }
        z_acc += my_z; // (a lane's share: at most 2^25 rows of |z| <= 128 each)
        for (int t = 0; t < m; t++) {
            const int slot = __shfl(my_slot, t), k = __shfl(my_sym, t);
            if (slot >= 0)
                acc += P.pi[(int64_t)slot * 64 + (int)((inverse >> (8 * k)) & 63u)];
        }
    }
}
__device__ __forceinline__ int64_t wave_sum(int64_t x)
{
    for (int off = 32; off; off >>= 1)
        x += __shfl_xor(x, off);
    return x;
}
__device__ __forceinline__ int64_t checked_groups(const iago_replay_merge_args &P)
{
    const int64_t groups = *P.n_unique;
    return groups < 0 ? 0 : groups > P.count ? P.count : groups;
}

// The large groups, spread: one wave per chunk of CHUNK sorted rows sums what the chunk holds of every group of more
// than SPREAD rows and adds it, with 64-bit integer atomics, into the group's 65 accumulators -- its 64 cells and its
// results -- which live in workspace[first[g] .. first[g] + 64], entries of the sorted order that are the group's own
// (the entry zeroes the workspace).  A window of twenty rounds holds the start position twenty thousand times: one
// wave would walk those rows alone while the device idles.  Integer sums: the order of the adds does not show.
__global__ __launch_bounds__(BLOCK) void merge_spread_kernel(const iago_replay_merge_args P)
{
    const int lane = threadIdx.x & 63;
    const int64_t count = P.count, groups = checked_groups(P);
    if (groups == 0)
        return;
    const uint64_t inverse = act_variant_inverse_all(lane);
    const int64_t stride = (int64_t)gridDim.x * ROWS;
    for (int64_t chunk = (int64_t)blockIdx.x * ROWS + (threadIdx.x >> 6); chunk * CHUNK < count; chunk += stride) {
        const int64_t cs = chunk * CHUNK, ce = cs + CHUNK < count ? cs + CHUNK : count;
        bool any = false; // (most chunks hold no row of a spread group: the lanes look at four rows each)
        for (int64_t i = cs + lane; i < ce; i += 64) {
            const int64_t g = P.group[i];
            if (g >= 0 && g < groups) {
                const Span s = group_span(P, g, groups);
                any |= s.end - s.start > SPREAD;
            }
        }
        if (!__any(any))
            continue;
        int64_t pos = cs;
        while (pos < ce) { // (pos and everything derived from it are the same in every lane)
            const int64_t g = P.group[pos];
            if (g < 0 || g >= groups) {
                pos++;
                continue;
            }
            const Span s = group_span(P, g, groups);
            int64_t to = s.end < ce ? s.end : ce;
            to = to <= pos ? pos + 1 : to; // (forward whatever first[] holds)
            if (s.end - s.start > SPREAD && s.start <= pos && pos < s.end) {
                uint64_t key_o, key_p;
                group_key(P, s.start, key_o, key_p);
                int64_t acc = 0;
                int z_acc = 0;
                bool bad = false;
                sum_rows(P, pos, to, key_o, key_p, inverse, lane, acc, z_acc, bad);
                const int64_t z_all = wave_sum(z_acc);
                // (s.start + 64 < s.end <= count: inside the workspace)
                atomicAdd((unsigned long long *)&P.workspace[s.start + lane], (unsigned long long)acc);
                if (lane == 0)
                    atomicAdd((unsigned long long *)&P.workspace[s.start + 64], (unsigned long long)z_all);
                if (bad)
                    atomicOr(P.flags, (uint32_t)IAGO_REPLAY_MERGE_BAD_INPUT);
            }
            pos = to;
        }
    }
}

// One wave per group, lane = canonical cell: the wave sums the group's rows itself, or takes the sums of
// merge_spread_kernel where the group was spread.  Sums in 64 bits, clamped to int32 on the way out (bit 1).  Plain
// stores.
__global__ __launch_bounds__(BLOCK) void merge_reduce_kernel(const iago_replay_merge_args P)
{
    const int lane = threadIdx.x & 63;
    const int64_t groups = checked_groups(P);
    const uint64_t inverse = act_variant_inverse_all(lane);
    const int64_t stride = (int64_t)gridDim.x * ROWS;
    for (int64_t g = (int64_t)blockIdx.x * ROWS + (threadIdx.x >> 6); g < groups; g += stride) {
        const Span s = group_span(P, g, groups);
        uint64_t key_o, key_p;
        group_key(P, s.start, key_o, key_p);
        int64_t acc = 0, z_all;
        if (s.end - s.start > SPREAD) {
            acc = P.workspace[s.start + lane];
            z_all = P.workspace[s.start + 64];
        } else {
            int z_acc = 0;
            bool bad = false;
            sum_rows(P, s.start, s.end, key_o, key_p, inverse, lane, acc, z_acc, bad);
            z_all = wave_sum(z_acc);
            if (bad)
                atomicOr(P.flags, (uint32_t)IAGO_REPLAY_MERGE_BAD_INPUT);
        }
        if (acc != clamp_i32(acc) || z_all != clamp_i32(z_all))
            atomicOr(P.flags, (uint32_t)IAGO_REPLAY_MERGE_OVERFLOW);
        P.pi_out[g * 64 + lane] = (int32_t)clamp_i32(acc);
        if (lane != 0)
            continue;
        P.own_out[g] = key_o;
        P.opp_out[g] = key_p;
        P.z_sum[g] = (int32_t)clamp_i32(z_all);
        P.mult[g] = (int32_t)(s.end - s.start);
    }
}

// iago_replay_sample's wave per output row over the merged rows: the group drawn uniformly over the groups, or over
// the window's rows and found by binary search on first[] (the last group that starts at or before the row).
__global__ __launch_bounds__(BLOCK) void replay_sample_merged_kernel(const iago_replay_sample_merged_args P)
{
    const int lane = threadIdx.x & 63;
    const uint32_t key0 = (uint32_t)P.seed, key1 = (uint32_t)(P.seed >> 32) ^ REPLAY_KEY;
    const uint32_t groups = (uint32_t)P.n_unique;
    const int64_t stride = (int64_t)gridDim.x * ROWS;
    for (int64_t j = (int64_t)blockIdx.x * ROWS + (threadIdx.x >> 6); j < P.n; j += stride) {
        uint32_t c[4] = {(uint32_t)j, P.step, 0u, 0u};
        philox4x32_10(c, key0, key1);
        const int k = (int)(c[1] & 7u);
        uint32_t g;
        if (P.mode == IAGO_REPLAY_MERGED_UNIQUE) {
            g = __umulhi(c[0], groups);
        } else {
            const int64_t r = (int64_t)__umulhi(c[0], (uint32_t)P.count);
            uint32_t lo = 0u, hi = groups; // first[lo] <= r (first[0] = 0) and lo < hi throughout: g stays < n_unique
            while (hi - lo > 1u) {
                const uint32_t mid = lo + (hi - lo) / 2u;
                if (P.first[mid] <= r)
                    lo = mid;
                else
                    hi = mid;
            }
            g = lo;
        }
        g = (uint32_t)__builtin_amdgcn_readfirstlane((int)g); // (the same in every lane: say so)
        P.pi_out[j * 64 + lane] = P.pi[(int64_t)g * 64 + act_variant_inverse(lane, k)];
        if (lane != 0)
            continue;
        const int32_t zs = P.z_sum[g], mu = P.mult[g];
        P.own_out[j] = bb_variant(P.own[g], k);
        P.opp_out[j] = bb_variant(P.opp[g], k);
        P.result_out[j] = (float)zs / (float)mu; // (one conversion each, one correctly rounded division)
        P.z_sum_out[j] = zs;
        P.mult_out[j] = mu;
        P.group_out[j] = (int32_t)g;
        P.sym_out[j] = (uint8_t)k;
    }
}

// iago_replay_merge_values: one wave per group, the lanes striding over the group's sorted rows, each summing the
// column's entries of its rows' slots in 64 bits; one 64-bit wave reduction; lane 0 stores.  Integer sums and plain
// stores: the bits do not depend on the schedule.  The span is clamped into the sorted order; a row whose slot lies
// outside [0, count) or whose group number is not g is left out (bit 0).
__global__ __launch_bounds__(BLOCK) void merge_values_kernel(const iago_replay_merge_values_args P)
{
    const int lane = threadIdx.x & 63;
    const int64_t count = P.count, stride = (int64_t)gridDim.x * ROWS;
    for (int64_t g = (int64_t)blockIdx.x * ROWS + (threadIdx.x >> 6); g < P.n_unique; g += stride) {
        int64_t start = P.first[g], len = P.mult[g];
        bool bad = start < 0 || start >= count || len < 1 || len > count - start;
        start = start < 0 ? 0 : start > count ? count : start;
        len = len < 0 ? 0 : len > count - start ? count - start : len;
        int64_t acc = 0;
        for (int64_t i = start + lane; i < start + len; i += 64) {
            const int slot = P.order[i];
            if ((uint32_t)slot < (uint32_t)count && (int64_t)P.group[i] == g) // (count < 2^31)
                acc += P.v[slot];
            else
                bad = true;
        }
        acc = wave_sum(acc);
        if (bad && P.flags)
            atomicOr(P.flags, (uint32_t)IAGO_REPLAY_MERGE_BAD_INPUT);
        if (lane == 0)
            P.v_sum[g] = acc;
    }
}

// iago_value_targets: one lane per game, walking its T turns backward; row t of every [t][b] record is contiguous over
// the games, so a wave's loads are.  The chain (Gnext, Vnext) lives in two 64-bit registers per lane: no LDS, no scratch.
// mover[t] is the same for every lane.  The rule: include/iago_hip_training.h.
__device__ __forceinline__ void value_targets_game(const iago_value_targets_args &P, int64_t b, int64_t lam, int64_t mix,
                                                   int64_t one)
{
    int64_t g_next = one * (int64_t)P.z[b], v_next = g_next;
    for (int64_t t = P.n_turns - 1; t >= 0; t--) {
        const int64_t at = t * P.n_games + b;
        const int kind = P.valid[at];
        const int64_t s = P.mover[t] == 1 ? 1 : -1;
        int32_t out = 0;
        if (kind == 1 || kind == 4 || kind == 3) {
            int64_t v;
            if (kind == 3) {
                const int sc = P.score[at];
                v = one * (int64_t)((sc > 0) - (sc < 0));
            } else {
                const int64_t q = P.q[at];
                v = q > one ? one : q < -one ? -one : q;
            }
            v *= s;
            const int64_t g = ((256 - lam) * v_next + lam * g_next + 128) >> 8; // (arithmetic: floors)
            const int64_t r = ((256 - mix) * g + mix * v + 128) >> 8;
            out = (int32_t)(s * r);
            g_next = g;
            v_next = v;
        }
        P.out[at] = out;
    }
}
__global__ __launch_bounds__(BLOCK) void value_targets_kernel(const iago_value_targets_args P)
{
    const int64_t lam = P.lam_256, mix = P.mix_256, one = 65536;
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (int64_t b = (int64_t)blockIdx.x * BLOCK + threadIdx.x; b < P.n_games; b += stride)
        value_targets_game(P, b, lam, mix, one);
}

unsigned grid_for(int64_t items, int per_block)
{
    const int64_t blocks = (items + per_block - 1) / per_block;
    return blocks < (int64_t)MAX_GRID ? (unsigned)blocks : MAX_GRID;
}

} // namespace

extern "C" {

int iago_replay_sample(const iago_replay_sample_args *args, void *stream)
{
    if (!args)
        return iago_fail(IAGO_ERR_INVALID, "iago_replay_sample: null args");
    const iago_replay_sample_args &A = *args;
    if (!A.own || !A.opp || !A.pi || !A.move || !A.z || !A.own_out || !A.opp_out || !A.pi_out || !A.move_out || !A.z_out)
        return iago_fail(IAGO_ERR_INVALID, "iago_replay_sample: null pointer");
    if (A.n <= 0)
        return iago_fail(IAGO_ERR_INVALID, "iago_replay_sample: n must be positive");
    if (A.count <= 0 || A.count > A.capacity || A.capacity >= ((int64_t)1 << 31))
        return iago_fail(IAGO_ERR_INVALID, "iago_replay_sample: need 1 <= count <= capacity < 2^31");
    if ((A.slot_in == nullptr) != (A.sym_in == nullptr))
        return iago_fail(IAGO_ERR_INVALID, "iago_replay_sample: slot_in and sym_in go together (both or neither)");
    const int64_t groups = (A.n + ROWS - 1) / ROWS;
    const unsigned grid = groups < (int64_t)MAX_GRID ? (unsigned)groups : MAX_GRID;
    hipLaunchKernelGGL(replay_sample_kernel, dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, A);
    return iago_check_launch("iago_replay_sample");
}

int iago_canonical_rows(const uint64_t *own, const uint64_t *opp, int64_t n, uint64_t *c_own, uint64_t *c_opp,
                        uint8_t *sym, void *stream)
{
    if (!own || !opp || !c_own || !c_opp || !sym)
        return iago_fail(IAGO_ERR_INVALID, "iago_canonical_rows: null pointer");
    if (n <= 0)
        return iago_fail(IAGO_ERR_INVALID, "iago_canonical_rows: n must be positive");
    hipLaunchKernelGGL(canonical_rows_kernel, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, own, opp, n,
                       c_own, c_opp, sym);
    return iago_check_launch("iago_canonical_rows");
}

int iago_replay_merge(const iago_replay_merge_args *args, void *stream)
{
    if (!args)
        return iago_fail(IAGO_ERR_INVALID, "iago_replay_merge: null args");
    const iago_replay_merge_args &A = *args;
    if (!A.c_own || !A.c_opp || !A.sym || !A.pi || !A.z || !A.order || !A.group || !A.own_out || !A.opp_out ||
        !A.pi_out || !A.z_sum || !A.mult || !A.first || !A.workspace || !A.n_unique || !A.flags)
        return iago_fail(IAGO_ERR_INVALID, "iago_replay_merge: null pointer");
    if (A.count <= 0 || A.count >= ((int64_t)1 << 31))
        return iago_fail(IAGO_ERR_INVALID, "iago_replay_merge: need 1 <= count < 2^31");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(A.workspace, 0, (size_t)A.count * sizeof(int64_t), s) != hipSuccess)
        return iago_fail(IAGO_ERR_HIP, "iago_replay_merge: clearing the workspace failed");
    hipLaunchKernelGGL(merge_heads_kernel, dim3(grid_for(A.count, BLOCK)), dim3(BLOCK), 0, s, A);
    hipLaunchKernelGGL(merge_count_kernel, dim3(1), dim3(1), 0, s, A);
    hipLaunchKernelGGL(merge_spread_kernel, dim3(grid_for((A.count + CHUNK - 1) / CHUNK, ROWS)), dim3(BLOCK), 0, s, A);
    hipLaunchKernelGGL(merge_reduce_kernel, dim3(grid_for(A.count, ROWS)), dim3(BLOCK), 0, s, A);
    return iago_check_launch("iago_replay_merge");
}

int iago_replay_sample_merged(const iago_replay_sample_merged_args *args, void *stream)
{
    if (!args)
        return iago_fail(IAGO_ERR_INVALID, "iago_replay_sample_merged: null args");
    const iago_replay_sample_merged_args &A = *args;
    if (!A.own || !A.opp || !A.pi || !A.z_sum || !A.mult || !A.first || !A.own_out || !A.opp_out || !A.pi_out ||
        !A.result_out || !A.z_sum_out || !A.mult_out || !A.group_out || !A.sym_out)
        return iago_fail(IAGO_ERR_INVALID, "iago_replay_sample_merged: null pointer");
    if (A.n <= 0)
        return iago_fail(IAGO_ERR_INVALID, "iago_replay_sample_merged: n must be positive");
    if (A.n_unique <= 0 || A.n_unique > A.count || A.count >= ((int64_t)1 << 31))
        return iago_fail(IAGO_ERR_INVALID, "iago_replay_sample_merged: need 1 <= n_unique <= count < 2^31");
    if (A.mode != IAGO_REPLAY_MERGED_UNIQUE && A.mode != IAGO_REPLAY_MERGED_ROWS)
        return iago_fail(IAGO_ERR_INVALID, "iago_replay_sample_merged: mode must be 0 (unique) or 1 (rows)");
    hipLaunchKernelGGL(replay_sample_merged_kernel, dim3(grid_for(A.n, ROWS)), dim3(BLOCK), 0, (hipStream_t)stream, A);
    return iago_check_launch("iago_replay_sample_merged");
}

int iago_replay_merge_values(const iago_replay_merge_values_args *args, void *stream)
{
    if (!args)
        return iago_fail(IAGO_ERR_INVALID, "iago_replay_merge_values: null args");
    const iago_replay_merge_values_args &A = *args;
    if (!A.order || !A.group || !A.first || !A.mult || !A.v || !A.v_sum)
        return iago_fail(IAGO_ERR_INVALID, "iago_replay_merge_values: null pointer");
    if (A.count <= 0 || A.count >= ((int64_t)1 << 31) || A.n_unique <= 0 || A.n_unique > A.count)
        return iago_fail(IAGO_ERR_INVALID, "iago_replay_merge_values: need 1 <= n_unique <= count < 2^31");
    hipLaunchKernelGGL(merge_values_kernel, dim3(grid_for(A.n_unique, ROWS)), dim3(BLOCK), 0, (hipStream_t)stream, A);
    return iago_check_launch("iago_replay_merge_values");
}

int iago_value_targets(const iago_value_targets_args *args, void *stream)
{
    if (!args)
        return iago_fail(IAGO_ERR_INVALID, "iago_value_targets: null args");
    const iago_value_targets_args &A = *args;
    if (!A.valid || !A.q || !A.score || !A.z || !A.mover || !A.out)
        return iago_fail(IAGO_ERR_INVALID, "iago_value_targets: null pointer");
    if (A.n_turns <= 0 || A.n_games <= 0 || A.n_turns > ((int64_t)1 << 31) / A.n_games)
        return iago_fail(IAGO_ERR_INVALID, "iago_value_targets: need n_turns >= 1, n_games >= 1, n_turns * n_games <= 2^31");
    if (A.lam_256 < 0 || A.lam_256 > 256 || A.mix_256 < 0 || A.mix_256 > 256)
        return iago_fail(IAGO_ERR_INVALID, "iago_value_targets: lam_256 and mix_256 must be in [0, 256]");
    hipLaunchKernelGGL(value_targets_kernel, dim3(grid_for(A.n_games, BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, A);
    return iago_check_launch("iago_value_targets");
}

} // extern "C"
