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

} // extern "C"
