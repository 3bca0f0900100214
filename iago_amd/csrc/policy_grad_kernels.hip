// policy_grad_kernels.hip -- the gradients of the REINFORCE update of SLPolicy (src/train_rl.py:55-66: pred =
// model(x) -- softmax probabilities --, loss = mean(softmax_cross_entropy(pred, y) * r), backward) on the f16 matrix
// units in "split f16" arithmetic: every float32 operand as two f16 numbers (22 significant bits), three MFMAs per
// product sum into float32 accumulators (csrc/conv_kernels.hip).  Together with iago_conv3x3_split (forward and,
// with transposed weights, backward-data) this replaces the MIOpen float32 convolutions of the update
// (9 ms of an 18 ms set at 1,900 rows: DESIGN.md section 5).  The Value net's supervised update (train_value.py:53-57,
// iago_value_mse_grad) runs the same trunk (pg_trunk_grad) with its own head kernels.
//
// Data: split channel blocks [n][C/16][64][16] f16 hi / lo as everywhere in conv_kernels.hip.  A gradient tensor
// carries a power-of-two scale 2^e (an int32 device word per tensor) so that its largest element sits near 2^14: the
// f16 pieces then hold 22 bits of every element down to 2^-28 of the largest (float32 keeps 24 of all of them; what
// is lost lies below the rounding of the sums the large elements dominate).
//
// wgrad_split_kernel: dW[co][ci][ky][kx] = sum over boards and cells of dY[b][co][y][x] * X[b][ci][y+ky-1][x+kx-1].
//   GEMM M = co, N = (ci, tap), K = (board, cell).  The operands live in memory with the CHANNELS innermost -- the
//   contraction runs over cells -- so both MFMA operands come out of LDS through ds_read_b64_tr_b16 (gfx950's
//   transposed read: a lane gets 4 consecutive cells of ONE channel).  One workgroup = 64 output channels x 32 input
//   channels x 9 taps (72 tiles of v_mfma_f32_16x16x32_f16, 18 per wave, 144 accumulator registers) over a group of
//   boards; a board is one stage (K = 64 = two k-steps), double-buffered in LDS.
//   Partial sums per group of boards go to memory and are added up in a fixed order (deterministic).
#include "abi_common.hpp"
#include "../../include/iago_hip_training.h"

#include <hip/hip_fp16.h>
#include <math.h>
#include <string>

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float float4v __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef short short4v __attribute__((__vector_size__(8)));
typedef __attribute__((address_space(3))) short4v lds_short4v;

// (through the builtin: a first form of this loop fed MFMAs from VALU results -- v_perm windows, register copies --, and
// the compiler only keeps the wait states of that right when it knows the instruction: the asm form of the walks gave
// wrong sums there.  The ISA has no accumulator copies in the loop: 108 MFMAs, 88 transposed reads per board and wave)
#define PG_MFMA16(acc, a, b) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc, 0, 0, 0)

// LDS images of one board: rows of 8 (dY) or 12 (X, padded: columns 0 and 9 are the zero border, 10 and 11 filler)
// cells x 32 B (16 channels), 384 B apart: the two 16-lane groups of a 32-lane half read rows that are one board row
// apart -- 96 banks = 32 mod 64 further, so their 128-byte blocks never share a bank
constexpr int WG_ROWB = 384;
constexpr int WG_DY_CB = 8 * WG_ROWB;       // one channel block of dY: 3,072 B
constexpr int WG_DY_PIECE = 4 * WG_DY_CB;   // hi or lo of the workgroup's 64 output channels: 12,288 B
constexpr int WG_X_CB = 10 * WG_ROWB;       // one channel block of the padded input: 3,840 B
constexpr int WG_X_PIECE = 2 * WG_X_CB;     // hi or lo of the workgroup's 32 input channels: 7,680 B
constexpr int WG_X_AT = 2 * WG_DY_PIECE;    // 24,576
constexpr int WG_BUF = WG_X_AT + 2 * WG_X_PIECE; // 39,936 B per board
constexpr int WG_LDS = 2 * WG_BUF;          // 79,872 B

struct WgradParams {
    const u32x4 *dy_hi, *dy_lo; // [n][8][64][16] f16: dL / d(pre-activation), times 2^e
    const u32x4 *x_hi, *x_lo;   // [n][cin/16][64][16] f16: the layer's input
    float *part;                // [groups][9][128][cin]
    int64_t n;
    int32_t cin, groups;
};

extern __shared__ __align__(16) char pg_lds[];

__device__ __forceinline__ uint2 lds_tr(int off)
{
    const short4v v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_short4v *)(pg_lds + off));
    return __builtin_bit_cast(uint2, v);
}

__device__ __forceinline__ half8 cat8(uint2 a, uint2 b)
{
    u32x4 v;
    v[0] = a.x, v[1] = a.y, v[2] = b.x, v[3] = b.y;
    return __builtin_bit_cast(half8, v);
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void wgrad_split_kernel(WgradParams P)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // the workgroups of one group of boards sit on ONE XCD (workgroup i runs on XCD i mod 8; groups is a multiple of
    // 8): they read the same boards at about the same time, through one L2
    const int group = (int)(blockIdx.x % (unsigned)P.groups), sub = (int)(blockIdx.x / (unsigned)P.groups);
    const int co_half = sub & 1, ciq = sub >> 1;
    const int mh = wv & 1, cbl = wv >> 1; // the wave's 32 of the 64 output channels, its 16 of the 32 input channels
    const int ncb = P.cin >> 4;
    const int64_t per = (P.n + P.groups - 1) / P.groups;
    const int64_t b_lo = group * per, b_hi = b_lo + per < P.n ? b_lo + per : P.n;

    for (int i = tid; i < 2 * WG_X_PIECE / 16; i += 256) { // the borders of the padded planes stay zero
        ((uint4 *)(pg_lds + WG_X_AT))[i] = make_uint4(0, 0, 0, 0);
        ((uint4 *)(pg_lds + WG_BUF + WG_X_AT))[i] = make_uint4(0, 0, 0, 0);
    }
    __syncthreads(); // (the first board's cells are written by OTHER threads than the ones that zeroed them)
    // staging: per board 1,024 16-byte pieces of dY (4 channel blocks x 64 cells x 2 halves x hi / lo) and 512 of X
    int dy_src[2], dy_dst[2];
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const int e = tid + 256 * q, cb = e >> 7, cell = (e >> 1) & 63, hp = e & 1;
        dy_src[q] = (co_half * 4 + cb) * 128 + (e & 127);
        dy_dst[q] = cb * WG_DY_CB + (cell >> 3) * WG_ROWB + (cell & 7) * 32 + hp * 16;
    }
    int x_src, x_dst;
    {
        const int e = tid, cb = e >> 7, cell = (e >> 1) & 63, hp = e & 1;
        x_src = (ciq * 2 + cb) * 128 + (e & 127);
        x_dst = WG_X_AT + cb * WG_X_CB + ((cell >> 3) + 1) * WG_ROWB + ((cell & 7) + 1) * 32 + hp * 16;
    }
    struct Staged {
        u32x4 v[6];
    };
    auto fetch = [&](int64_t b) {
        Staged G;
        G.v[0] = P.dy_hi[b * 1024 + dy_src[0]];
        G.v[1] = P.dy_hi[b * 1024 + dy_src[1]];
        G.v[2] = P.dy_lo[b * 1024 + dy_src[0]];
        G.v[3] = P.dy_lo[b * 1024 + dy_src[1]];
        G.v[4] = P.x_hi[b * ncb * 128 + x_src];
        G.v[5] = P.x_lo[b * ncb * 128 + x_src];
        return G;
    };
    auto commit = [&](const Staged &G, int buf) {
        char *at = pg_lds + buf * WG_BUF;
        *(u32x4 *)(at + dy_dst[0]) = G.v[0];
        *(u32x4 *)(at + dy_dst[1]) = G.v[1];
        *(u32x4 *)(at + WG_DY_PIECE + dy_dst[0]) = G.v[2];
        *(u32x4 *)(at + WG_DY_PIECE + dy_dst[1]) = G.v[3];
        *(u32x4 *)(at + x_dst) = G.v[4];
        *(u32x4 *)(at + WG_X_PIECE + x_dst) = G.v[5];
    };

    float4v acc_m[2][9], acc_c[2][9];
#pragma unroll
    for (int mi = 0; mi < 2; mi++)
#pragma unroll
        for (int t = 0; t < 9; t++)
#pragma unroll
            for (int v = 0; v < 4; v++) {
                acc_m[mi][t][v] = 0.0f;
                acc_c[mi][t][v] = 0.0f;
            }

    // transposed reads: lane 4q + p of the 16-lane group kq supplies the address of row q (a cell), columns 4p .. 4p+3
    // (channels); lane i of the group receives channel i of the 4 cells.  k = 8 kq + j of k-step s <-> cell (row kq +
    // 4s, column j): two reads per operand (columns 0-3, 4-7).
    const int kq = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    const int lane_off = kq * WG_ROWB + q * 32 + p * 8;

    auto compute = [&](int buf) {
        const int at = buf * WG_BUF + lane_off;
        // A: this wave's two M tiles, both k-steps (16 reads); B: one (k-step, kernel row, kernel column) at a time --
        // the padded row kq + 4s + ky of this lane's channel, cells kx .. kx + 7: two transposed reads per piece (a
        // lane's rows may start anywhere: + 32 B per cell; windows cut out of one 12-cell read by v_alignbit and
        // register copies measured slower) -- read TWO steps ahead of the six MFMAs that use it
        half8 a_hi[2][2], a_lo[2][2];
#pragma unroll
        for (int s = 0; s < 2; s++)
#pragma unroll
            for (int mi = 0; mi < 2; mi++) {
                const int pa = at + (2 * mh + mi) * WG_DY_CB + 4 * s * WG_ROWB;
                a_hi[s][mi] = cat8(lds_tr(pa), lds_tr(pa + 128));
                a_lo[s][mi] = cat8(lds_tr(pa + WG_DY_PIECE), lds_tr(pa + WG_DY_PIECE + 128));
            }
        half8 b_hi[3], b_lo[3];
        auto load_b = [&](int step, int slot) {
            const int s = step / 9, ky = (step % 9) / 3, kx = step % 3;
            const int pb = at + WG_X_AT + cbl * WG_X_CB + (4 * s + ky) * WG_ROWB + 32 * kx;
            b_hi[slot] = cat8(lds_tr(pb), lds_tr(pb + 128));
            b_lo[slot] = cat8(lds_tr(pb + WG_X_PIECE), lds_tr(pb + WG_X_PIECE + 128));
        };
        load_b(0, 0);
        load_b(1, 1);
#pragma unroll
        for (int step = 0; step < 18; step++) {
            if (step + 2 < 18)
                load_b(step + 2, (step + 2) % 3);
            const int s = step / 9, t = step % 9, cur = step % 3;
            PG_MFMA16(acc_c[0][t], a_hi[s][0], b_lo[cur]);
            PG_MFMA16(acc_c[1][t], a_hi[s][1], b_lo[cur]);
            PG_MFMA16(acc_m[0][t], a_hi[s][0], b_hi[cur]);
            PG_MFMA16(acc_m[1][t], a_hi[s][1], b_hi[cur]);
            PG_MFMA16(acc_c[0][t], a_lo[s][0], b_hi[cur]);
            PG_MFMA16(acc_c[1][t], a_lo[s][1], b_hi[cur]);
        }
    };

    // Boards b + 1 .. b + 3 are on their way (registers) while board b is multiplied: one board is 0.75 us of MFMAs, a
    // load from beyond L2 takes longer than that under load.  Three register sets in rotation: the set of board b + 1
    // goes to the other LDS buffer right after board b's MFMAs, and is re-issued for board b + 4 at the next turn.
    if (b_lo < b_hi)
        commit(fetch(b_lo), 0);
    __syncthreads();
    const int64_t last = b_hi - 1;
    auto clamp = [&](int64_t b) { return b < last ? b : last; }; // (past the end: a harmless repeat, never committed)
    Staged S0, S1, S2;
    if (b_lo < b_hi) {
        S1 = fetch(clamp(b_lo + 1));
        S2 = fetch(clamp(b_lo + 2));
    }
    auto turn = [&](int64_t b, Staged &next, Staged &refill) {
        // next: board b + 1; refill: the set that held board b (committed a turn ago), now board b + 3
        refill = fetch(clamp(b + 3));
        compute((int)(b - b_lo) & 1);
        if (b + 1 < b_hi)
            commit(next, ((int)(b - b_lo) & 1) ^ 1);
        __syncthreads();
    };
    for (int64_t b = b_lo; b < b_hi; b += 3) {
        turn(b, S1, S0);
        if (b + 1 < b_hi)
            turn(b + 1, S2, S1);
        if (b + 2 < b_hi)
            turn(b + 2, S0, S2);
    }
    // tile (mi, tap): the lane holds rows 4 kq + v (output channels), column lane & 15 (input channel)
    const int ci = ciq * 32 + cbl * 16 + (lane & 15);
#pragma unroll
    for (int mi = 0; mi < 2; mi++)
#pragma unroll
        for (int t = 0; t < 9; t++)
#pragma unroll
            for (int v = 0; v < 4; v++) {
                const int co = co_half * 64 + (2 * mh + mi) * 16 + 4 * kq + v;
                P.part[(((int64_t)group * 9 + t) * 128 + co) * P.cin + ci] =
                    acc_m[mi][t][v] + acc_c[mi][t][v] * (1.0f / 2048.0f);
            }
}

// dW[co][ci][tap] = 2^-e * sum over the groups, in group order
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float *part, int groups, int cin, const int32_t *scale_exp,
                                                           float *dw)
{
    const int t = blockIdx.x * 256 + threadIdx.x; // (tap, co, ci)
    const int total = 9 * 128 * cin;
    if (t >= total)
        return;
    float s = 0.0f;
    for (int g = 0; g < groups; g++)
        s += part[(int64_t)g * total + t];
    if (scale_exp)
        s = ldexpf(s, -*scale_exp);
    const int ci = t % cin, co = (t / cin) & 127, tap = t / (cin * 128);
    dw[((int64_t)co * cin + ci) * 9 + tap] = s;
}


// The partial sums of ALL blocks of an update in one launch (iago_policy_reinforce_grad): per block k the weight gradient's
// groups (wgrad_reduce_kernel's arithmetic: the groups in order, then 2^-e) and the bias gradient's pair sums
// (bias_reduce_kernel's, conv_kernels.hip: a wave per channel, lane l takes boards l, l + 64, .., then the xor tree) -- the
// same sums in the same order as the per-block launches, which were 14 launches of mostly latency (23 us per block).
__device__ __forceinline__ float wave_sum_xor(float v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
        v += __shfl_xor(v, d);
    return v;
}
struct ReduceAllParams {
    const float *wpart[7], *bpart[7];
    float *dw[7], *db[7];
    const int32_t *scale_exp[7];
    int32_t groups[7], cin[7];
    int32_t w_block0[8]; // first workgroup of block k's weights; [7] = first workgroup of the biases
    int64_t n;
};
__global__ __launch_bounds__(256) void grad_reduce_all_kernel(ReduceAllParams P)
{
    const int b = blockIdx.x;
    if (b < P.w_block0[7]) {
        int k = 0;
#pragma unroll
        for (int i = 1; i < 7; i++)
            k += b >= P.w_block0[i] ? 1 : 0;
        // (by-value parameter arrays indexed at run time go through scratch memory: select with compile-time indices)
        const float *part = P.wpart[0];
        float *dw = P.dw[0];
        const int32_t *se = P.scale_exp[0];
        int groups = P.groups[0], cin = P.cin[0], first = P.w_block0[0];
#pragma unroll
        for (int i = 1; i < 7; i++)
            if (k == i) {
                part = P.wpart[i], dw = P.dw[i], se = P.scale_exp[i];
                groups = P.groups[i], cin = P.cin[i], first = P.w_block0[i];
            }
        const int t = (b - first) * 256 + threadIdx.x; // (tap, co, ci)
        const int total = 9 * 128 * cin;
        if (t >= total)
            return;
        float s = 0.0f;
        for (int g = 0; g < groups; g++)
            s += part[(int64_t)g * total + t];
        s = ldexpf(s, -*se);
        const int ci = t % cin, co = (t / cin) & 127, tap = t / (cin * 128);
        dw[((int64_t)co * cin + ci) * 9 + tap] = s;
        return;
    }
    // biases: 4 channels per workgroup (a wave each), 128 channels per block
    const int j = (b - P.w_block0[7]) * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int k = j >> 7, ch = j & 127;
    if (k >= 7)
        return;
    const float *bp = P.bpart[0];
    float *db = P.db[0];
#pragma unroll
    for (int i = 1; i < 7; i++)
        if (k == i)
            bp = P.bpart[i], db = P.db[i];
    const int cb = ch >> 4, c = ch & 15;
    float s = 0.0f;
    for (int64_t bd = lane; bd < P.n; bd += 64) {
        const int64_t pair = bd * 8 + cb;
        s += bp[(pair >> 1) * 32 + (pair & 1) * 16 + c];
    }
    s = wave_sum_xor(s);
    if (lane == 0)
        db[ch] = s;
}

// ---- The head of SLPolicy and the loss, forward and backward in one pass (network.py:29-47, src/train_rl.py:61-64):
//   logits = conv9 (1x1, 128 -> 1, no bias) + bias10[cell];  p = softmax(logits)            (the model's output)
//   c = softmax_cross_entropy(p, a) = logsumexp(p) - p[a]     (the reference applies log-softmax to the probabilities)
//   loss = sum_b c_b z_b / n_true
// and back: g = (z / n_true) (softmax(p) - onehot(a)), dlogits = p (g - <g, p>), dW9[c] = sum dlogits x8[c],
// dbias10[cell] = sum dlogits, dY8[c][cell] = [x8 > 0] dlogits[cell] w9[c] (the gradient at block 8's pre-activations,
// float32 channel blocks + the largest magnitude).  One wave per board at a time, lane = cell; float32 arithmetic on
// the exact values hi + lo 2^-11.
struct HeadGradParams {
    const uint4 *x_hi, *x_lo;  // [n][8][64][16] f16: the output of block 8
    const float *w9, *b10;     // [128], [64]
    const int32_t *action;     // [n]
    const float *reward;       // [n]
    float inv_n;               // 1 / (rows the mean divides by)
    int64_t n;
    float4v *dy;               // [n][8][64][16] float32
    uint32_t *max_bits;
    float *part;               // [gridDim.x][193]: dW9 (128), dbias10 (64), loss (1) of each workgroup
    float *probs;              // optional [n][64]: the model's output
    uint32_t *bad;             // optional: bit 1 raised when an action is outside 0 .. 63 (F.softmax_cross_entropy would raise)
};
constexpr int HEAD_PART = 193;

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
        v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
        v = fmaxf(v, __shfl_xor(v, d));
    return v;
}

// ---- What the heads of SLPolicy's two losses share (head_grad_kernel, head_visits_grad_kernel): one wave per board,
// lane = cell
// x[c] = block 8's output at this lane's cell, the exact values hi + lo 2^-11
__device__ __forceinline__ void head_load_x8(const uint4 *x_hi, const uint4 *x_lo, int64_t b, int lane, float (&x)[128])
{
#pragma unroll
    for (int cb = 0; cb < 8; cb++) {
        const int64_t at = ((b * 8 + cb) * 64 + lane) * 2;
        const uint4 h0 = x_hi[at], h1 = x_hi[at + 1], l0 = x_lo[at], l1 = x_lo[at + 1];
        const __half2 *hh0 = (const __half2 *)&h0, *hh1 = (const __half2 *)&h1;
        const __half2 *ll0 = (const __half2 *)&l0, *ll1 = (const __half2 *)&l1;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float2 a = __half22float2(hh0[k]), c2 = __half22float2(ll0[k]);
            const float2 d = __half22float2(hh1[k]), e2 = __half22float2(ll1[k]);
            x[16 * cb + 2 * k] = a.x + c2.x * (1.0f / 2048.0f);
            x[16 * cb + 2 * k + 1] = a.y + c2.y * (1.0f / 2048.0f);
            x[16 * cb + 8 + 2 * k] = d.x + e2.x * (1.0f / 2048.0f);
            x[16 * cb + 8 + 2 * k + 1] = d.y + e2.y * (1.0f / 2048.0f);
        }
    }
}
// p = softmax(conv9 . x + bias10) over the board (F.softmax, network.py:46); shifted = logit - max logit and
// sum = sum exp(shifted): log p = shifted - log(sum)
__device__ __forceinline__ float head_softmax(const float *w9, const float (&x)[128], float my_b10, float &shifted,
                                              float &sum)
{
    float logit = 0.0f;
#pragma unroll
    for (int c = 0; c < 128; c++)
        logit = fmaf(w9[c], x[c], logit);
    logit += my_b10;
    shifted = logit - wave_max(logit);
    const float ex = expf(shifted);
    sum = wave_sum(ex);
    return ex / sum;
}
// dl = the loss's gradient at this cell's logit: acc9 += dl x (dW9), dY8 = [x8 > 0] dl w9 to dy, its largest magnitude
__device__ __forceinline__ void head_write_back(float dl, const float (&x)[128], const float *w9, float4v *dy, int64_t b,
                                                int lane, float (&acc9)[128], float &big)
{
#pragma unroll
    for (int cb = 0; cb < 8; cb++) {
#pragma unroll
        for (int qt = 0; qt < 4; qt++) {
            float4v v;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int c = 16 * cb + 4 * qt + k;
                acc9[c] = fmaf(dl, x[c], acc9[c]);
                v[k] = x[c] > 0.0f ? dl * w9[c] : 0.0f;
                big = fmaxf(big, fabsf(v[k]));
            }
            dy[((b * 8 + cb) * 64 + lane) * 4 + qt] = v;
        }
    }
}
// a workgroup's partial sums to part[blockIdx.x][HEAD_PART], the largest magnitude to max_bits
__device__ __forceinline__ void head_finish(float (*red)[HEAD_PART], const float (&acc9)[128], float acc_b,
                                            float acc_loss, float big, uint32_t *max_bits, float *part)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    big = wave_max(big);
    if (lane == 0 && big > 0.0f)
        atomicMax(max_bits, __float_as_uint(big));
#pragma unroll
    for (int c = 0; c < 128; c++) {
        const float s = wave_sum(acc9[c]);
        if (lane == 0)
            red[wv][c] = s;
    }
    red[wv][128 + lane] = acc_b;
    if (lane == 0)
        red[wv][192] = acc_loss; // (the same in every lane)
    __syncthreads();
    if (threadIdx.x < HEAD_PART)
        part[(int64_t)blockIdx.x * HEAD_PART + threadIdx.x] =
            red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

__global__ __launch_bounds__(256) void head_grad_kernel(HeadGradParams P)
{
    __shared__ float red[4][HEAD_PART];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float acc9[128];
#pragma unroll
    for (int c = 0; c < 128; c++)
        acc9[c] = 0.0f;
    float acc_b = 0.0f, acc_loss = 0.0f, big = 0.0f;
    const float my_b10 = P.b10[lane];
    for (int64_t b = (int64_t)blockIdx.x * 4 + wv; b < P.n; b += (int64_t)gridDim.x * 4) {
        float x[128], shifted, sum;
        head_load_x8(P.x_hi, P.x_lo, b, lane, x);
        const float p = head_softmax(P.w9, x, my_b10, shifted, sum);
        if (P.probs)
            P.probs[b * 64 + lane] = p;
        const int a = P.action[b];
        const float z = P.reward[b];
        if ((uint32_t)a >= 64u && lane == 0 && P.bad)
            atomicOr(P.bad, 2u); // (the row's loss and gradient mean nothing: the caller must not use this update)
        // F.softmax_cross_entropy(pred, y): log-softmax of the probabilities (src/train_rl.py:62)
        const float m2 = wave_max(p);
        const float ex2 = expf(p - m2);
        const float s2 = wave_sum(ex2);
        const float lse = m2 + logf(s2);
        const float p_a = __shfl(p, a & 63);
        acc_loss += (lse - p_a) * z;
        const float g = z * P.inv_n * (ex2 / s2 - (lane == a ? 1.0f : 0.0f));
        const float dl = p * (g - wave_sum(g * p));                 // through the model's softmax
        acc_b += dl;
        head_write_back(dl, x, P.w9, P.dy, b, lane, acc9, big);
    }
    head_finish(red, acc9, acc_b, acc_loss, big, P.max_bits, P.part);
}

// ---- The head of SLPolicy under the visit-count loss: the cross-entropy of the model's output (ONE softmax) against
// the search's visit distribution t = n / N of the row (engine.SelfPlayResult.tuples()["pi"]), weighted per row:
//   loss = sum_b w_b sum_{a: n[a] > 0} -t[a] log p[a] / n_mean,  log p = (logit - max) - log sum exp(logit - max)
//   dlogits = (w / n_mean) (p - t)
// (never logf(p): a cell whose p underflowed keeps a finite log p).  A row with N == 0 contributes nothing; so does a
// row with a negative count, which raises bit 1 of `bad` besides.  Launch shape, partial sums and dY8 as
// head_grad_kernel.
struct HeadVisitsGradParams {
    const uint4 *x_hi, *x_lo;  // [n][8][64][16] f16: the output of block 8
    const float *w9, *b10;     // [128], [64]
    const int32_t *visits;     // [n][64]
    const float *weight;       // optional [n] (NULL: 1)
    float inv_n;               // 1 / (rows the mean divides by)
    int64_t n;
    float4v *dy;               // [n][8][64][16] float32
    uint32_t *max_bits;
    float *part;               // [gridDim.x][193]: dW9 (128), dbias10 (64), loss (1) of each workgroup
    float *probs;              // optional [n][64]: the model's output
    uint32_t *bad;             // optional: bit 1 raised by a negative count
};

__global__ __launch_bounds__(256) void head_visits_grad_kernel(HeadVisitsGradParams P)
{
    __shared__ float red[4][HEAD_PART];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float acc9[128];
#pragma unroll
    for (int c = 0; c < 128; c++)
        acc9[c] = 0.0f;
    float acc_b = 0.0f, acc_loss = 0.0f, big = 0.0f;
    const float my_b10 = P.b10[lane];
    for (int64_t b = (int64_t)blockIdx.x * 4 + wv; b < P.n; b += (int64_t)gridDim.x * 4) {
        float x[128], shifted, sum;
        head_load_x8(P.x_hi, P.x_lo, b, lane, x);
        const float p = head_softmax(P.w9, x, my_b10, shifted, sum);
        if (P.probs)
            P.probs[b * 64 + lane] = p;
        const int32_t nv = P.visits[b * 64 + lane];
        const float w = P.weight ? P.weight[b] : 1.0f;
        int64_t total = nv;                                         // (64 bits: any int32 counts sum without wrapping)
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1)
            total += __shfl_xor(total, d);
        const bool negative = __ballot(nv < 0) != 0;
        if (negative && lane == 0 && P.bad)
            atomicOr(P.bad, 2u); // (the caller must not use this update)
        const bool live = total > 0 && !negative;
        const float t = live ? (float)nv / (float)total : 0.0f;
        acc_loss += w * wave_sum(t > 0.0f ? -t * (shifted - logf(sum)) : 0.0f);
        const float dl = live ? w * P.inv_n * (p - t) : 0.0f;
        acc_b += dl;
        head_write_back(dl, x, P.w9, P.dy, b, lane, acc9, big);
    }
    head_finish(red, acc9, acc_b, acc_loss, big, P.max_bits, P.part);
}

// out[j] = (j == 192 ? inv_n : 1) * sum over the workgroups' partial sums: one wave per output, lane l takes the partial
// sums l, l + 64, .. (a fixed order)
__global__ __launch_bounds__(256) void head_reduce_kernel(const float *part, int n_parts, float inv_n, float *dw9, float *db10,
                                                          float *loss)
{
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= HEAD_PART)
        return;
    float s = 0.0f;
    for (int i = lane; i < n_parts; i += 64)
        s += part[(int64_t)i * HEAD_PART + j];
    s = wave_sum(s);
    if (lane != 0)
        return;
    if (j < 128)
        dw9[j] = s;
    else if (j < 192)
        db10[j - 128] = s;
    else
        *loss = s * inv_n;
}

// ---- The head of the Value net and its loss, forward and backward (network.py:66-96, train_value.py:53-57):
//   h9 = relu(conv3x3(x8; w9) + b9), h10 = w10 . h9, d = h10 * mask (keep ? scale : 0), pred = w11 . d,
//   loss = sum (pred - y)^2 / n_mean, dpred = (2 / n_mean) (pred - y)
// and back: dw11 = sum dpred d, dh10 = dpred w11 mask, dh9 = w10^T dh10, dpre9 = [h9 > 0] dh9, db9 = sum dpre9,
// dY8[c][i] = [x8 > 0] sum_t w9[c][t] dpre9[i - t] (float32 channel blocks + the largest magnitude, as
// head_grad_kernel writes them).  One wave per board at a time, lane = cell; plain float32 arithmetic (the head is
// 0.13 % of the forward's products).  dw10 and dw9 need a product per board of all cells or all channels: they come
// from the per-board values this kernel keeps (h9, dh10, dpre9) in value_head_wgrad_kernel.
struct ValueHeadGradParams {
    const uint4 *x_hi, *x_lo;    // [n][8][64][16] f16: the output of block 8
    const float *w9, *b9, *w10, *w11;
    const float *result;         // [n]
    const uint8_t *keep;         // optional [n][128]
    float scale, two_over_n;
    int64_t n;
    float4v *dy;                 // [n][8][64][16] float32
    uint32_t *max_bits;
    float *h9, *dh10, *dpre9;    // [n][64], [n][128], [n][64]
    float *part;                 // [gridDim.x][VHEAD_PART]: dw11 (128), db9 (1), sum of squares (1) per workgroup
    float *pred, *h9_out;        // optional [n], [n][64]
};
constexpr int VHEAD_PART = 130;
constexpr int VW10_STRIDE = 129; // w10 in LDS as [cell][unit], rows padded: both walks conflict-free

__device__ __forceinline__ float lane_value(float v, int l)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

__global__ __launch_bounds__(256) void value_head_grad_kernel(ValueHeadGradParams P)
{
    __shared__ float w9s[9 * 128];            // [tap][channel]
    __shared__ float w10s[64 * VW10_STRIDE];  // [cell][unit]
    __shared__ float red[4][VHEAD_PART];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int i = tid; i < 9 * 128; i += 256)
        w9s[i] = P.w9[(i & 127) * 9 + (i >> 7)];
    for (int i = tid; i < 128 * 64; i += 256)
        w10s[(i & 63) * VW10_STRIDE + (i >> 6)] = P.w10[i];
    __syncthreads();
    const float b9 = P.b9[0], w11a = P.w11[lane], w11b = P.w11[lane + 64];
    const int y = lane >> 3, xc = lane & 7;
    float acc11a = 0.0f, acc11b = 0.0f, acc_b9 = 0.0f, acc_sq = 0.0f, big = 0.0f;
    for (int64_t b = (int64_t)blockIdx.x * 4 + wv; b < P.n; b += (int64_t)gridDim.x * 4) {
        // (the weights' LDS reads through an offset the compiler cannot see: hoisted out of the loop, all 9,344 of
        // them would live in registers and spill)
        int z = 0;
        asm volatile("" : "+v"(z));
        const float *w9l = w9s + z, *w10l = w10s + z;
        float x[128];
#pragma unroll
        for (int cb = 0; cb < 8; cb++) {
            const int64_t at = ((b * 8 + cb) * 64 + lane) * 2;
            const uint4 h0 = P.x_hi[at], h1 = P.x_hi[at + 1], l0 = P.x_lo[at], l1 = P.x_lo[at + 1];
            const __half2 *hh0 = (const __half2 *)&h0, *hh1 = (const __half2 *)&h1;
            const __half2 *ll0 = (const __half2 *)&l0, *ll1 = (const __half2 *)&l1;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float2 a = __half22float2(hh0[k]), c2 = __half22float2(ll0[k]);
                const float2 d = __half22float2(hh1[k]), e2 = __half22float2(ll1[k]);
                x[16 * cb + 2 * k] = a.x + c2.x * (1.0f / 2048.0f);
                x[16 * cb + 2 * k + 1] = a.y + c2.y * (1.0f / 2048.0f);
                x[16 * cb + 8 + 2 * k] = d.x + e2.x * (1.0f / 2048.0f);
                x[16 * cb + 8 + 2 * k + 1] = d.y + e2.y * (1.0f / 2048.0f);
            }
        }
        // block 9: this cell's term of every tap, gathered at the output cells; taps in order
        float pre = 0.0f;
#pragma unroll
        for (int t = 0; t < 9; t++) {
            float v = 0.0f;
#pragma unroll
            for (int c = 0; c < 128; c++)
                v = fmaf(w9l[t * 128 + c], x[c], v);
            const int yy = y + t / 3 - 1, xx = xc + t % 3 - 1;
            const bool in = yy >= 0 && yy < 8 && xx >= 0 && xx < 8;
            const float g = __shfl(v, in ? yy * 8 + xx : 0);
            pre += in ? g : 0.0f;
        }
        const float h9 = fmaxf(pre + b9, 0.0f);
        P.h9[b * 64 + lane] = h9;
        if (P.h9_out)
            P.h9_out[b * 64 + lane] = h9;
        // fc10 (units lane and lane + 64), the dropout mask, fc11
        float h10a = 0.0f, h10b = 0.0f;
#pragma unroll
        for (int c = 0; c < 64; c++) {
            const float hc = lane_value(h9, c);
            h10a = fmaf(w10l[c * VW10_STRIDE + lane], hc, h10a);
            h10b = fmaf(w10l[c * VW10_STRIDE + 64 + lane], hc, h10b);
        }
        float ma = 1.0f, mb = 1.0f;
        if (P.keep) {
            ma = P.keep[b * 128 + lane] ? P.scale : 0.0f;
            mb = P.keep[b * 128 + 64 + lane] ? P.scale : 0.0f;
        }
        const float da = h10a * ma, db = h10b * mb;
        const float pred = wave_sum(fmaf(w11b, db, w11a * da));
        if (P.pred && lane == 0)
            P.pred[b] = pred;
        const float diff = pred - P.result[b];
        acc_sq = fmaf(diff, diff, acc_sq); // (the same in every lane)
        const float dp = P.two_over_n * diff;
        acc11a = fmaf(dp, da, acc11a);
        acc11b = fmaf(dp, db, acc11b);
        const float dha = dp * w11a * ma, dhb = dp * w11b * mb;
        P.dh10[b * 128 + lane] = dha;
        P.dh10[b * 128 + 64 + lane] = dhb;
        // back through fc10 to this cell, then block 9's ReLU
        float dh9 = 0.0f;
#pragma unroll
        for (int j = 0; j < 64; j++)
            dh9 = fmaf(w10l[lane * VW10_STRIDE + j], lane_value(dha, j), dh9);
#pragma unroll
        for (int j = 0; j < 64; j++)
            dh9 = fmaf(w10l[lane * VW10_STRIDE + 64 + j], lane_value(dhb, j), dh9);
        const float dpre = h9 > 0.0f ? dh9 : 0.0f;
        acc_b9 += dpre;
        P.dpre9[b * 64 + lane] = dpre;
        // block 9 transposed: input cell i takes dpre9 of output cell i - tap
        float g[9];
#pragma unroll
        for (int t = 0; t < 9; t++) {
            const int yy = y - t / 3 + 1, xx = xc - t % 3 + 1;
            const bool in = yy >= 0 && yy < 8 && xx >= 0 && xx < 8;
            const float s = __shfl(dpre, in ? yy * 8 + xx : 0);
            g[t] = in ? s : 0.0f;
        }
#pragma unroll
        for (int cb = 0; cb < 8; cb++) {
#pragma unroll
            for (int qt = 0; qt < 4; qt++) {
                float4v v;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int c = 16 * cb + 4 * qt + k;
                    float s = 0.0f;
#pragma unroll
                    for (int t = 0; t < 9; t++)
                        s = fmaf(w9l[t * 128 + c], g[t], s);
                    v[k] = x[c] > 0.0f ? s : 0.0f;
                    big = fmaxf(big, fabsf(v[k]));
                }
                P.dy[((b * 8 + cb) * 64 + lane) * 4 + qt] = v;
            }
        }
    }
    big = wave_max(big);
    if (lane == 0 && big > 0.0f)
        atomicMax(P.max_bits, __float_as_uint(big));
    acc_b9 = wave_sum(acc_b9);
    red[wv][lane] = acc11a;
    red[wv][64 + lane] = acc11b;
    if (lane == 0) {
        red[wv][128] = acc_b9;
        red[wv][129] = acc_sq;
    }
    __syncthreads();
    if (tid < VHEAD_PART)
        P.part[(int64_t)blockIdx.x * VHEAD_PART + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
}

// dw10[j][c] = sum dh10[j] h9[c] and dw9[c][tap] = sum over output cells o of dpre9[o] x8[c][o + tap], per workgroup
// over a contiguous range of boards (in board order); one board at a time in LDS
constexpr int VW_PART = 128 * 64 + 128 * 9;
constexpr int VX_STRIDE = 65;
struct ValueWgradParams {
    const uint4 *x_hi, *x_lo;
    const float *h9, *dh10, *dpre9;
    int64_t n;
    float *part;                 // [gridDim.x][VW_PART]: dw10 [128][64], dw9 [128][9]
};

template <int T0, int NT>
__device__ __forceinline__ void value_w9_taps(float (&acc)[5], const float *xs, const float *dps)
{
#pragma unroll
    for (int i = 0; i < NT; i++) {
        const int ky = (T0 + i) / 3, kx = (T0 + i) % 3;
        float s = acc[i];
#pragma unroll
        for (int o = 0; o < 64; o++) {
            const int yy = (o >> 3) + ky - 1, xx = (o & 7) + kx - 1;
            if (yy >= 0 && yy < 8 && xx >= 0 && xx < 8)
                s = fmaf(dps[o], xs[yy * 8 + xx], s);
        }
        acc[i] = s;
    }
}

__global__ __launch_bounds__(256) void value_head_wgrad_kernel(ValueWgradParams P)
{
    __shared__ float xs[128 * VX_STRIDE]; // [channel][cell]
    __shared__ float hs[64], dps[64], ds[128];
    const int tid = threadIdx.x;
    const int64_t per = (P.n + gridDim.x - 1) / gridDim.x;
    const int64_t b_lo = (int64_t)blockIdx.x * per, b_hi = b_lo + per < P.n ? b_lo + per : P.n;
    const int j = tid >> 1, c0 = (tid & 1) * 32, c = tid & 127;
    float a10[32], a9[5];
#pragma unroll
    for (int k = 0; k < 32; k++)
        a10[k] = 0.0f;
#pragma unroll
    for (int k = 0; k < 5; k++)
        a9[k] = 0.0f;
    for (int64_t b = b_lo; b < b_hi; b++) {
#pragma unroll
        for (int q = 0; q < 4; q++) { // 1,024 pieces of 8 channels: (block, cell, half)
            const int e = tid + 256 * q, cb = e >> 7, cell = (e >> 1) & 63, hp = e & 1;
            const uint4 h = P.x_hi[b * 1024 + e], l = P.x_lo[b * 1024 + e];
            const __half2 *hh = (const __half2 *)&h, *ll = (const __half2 *)&l;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float2 a = __half22float2(hh[k]), d = __half22float2(ll[k]);
                const int ch = cb * 16 + hp * 8 + 2 * k;
                xs[ch * VX_STRIDE + cell] = a.x + d.x * (1.0f / 2048.0f);
                xs[(ch + 1) * VX_STRIDE + cell] = a.y + d.y * (1.0f / 2048.0f);
            }
        }
        if (tid < 64) {
            hs[tid] = P.h9[b * 64 + tid];
            dps[tid] = P.dpre9[b * 64 + tid];
        } else if (tid < 192) {
            ds[tid - 64] = P.dh10[b * 128 + tid - 64];
        }
        __syncthreads();
        const float g = ds[j];
#pragma unroll
        for (int k = 0; k < 32; k++)
            a10[k] = fmaf(g, hs[c0 + k], a10[k]);
        if (tid < 128) // (wave-uniform)
            value_w9_taps<0, 5>(a9, xs + c * VX_STRIDE, dps);
        else
            value_w9_taps<5, 4>(a9, xs + c * VX_STRIDE, dps);
        __syncthreads();
    }
    float *out = P.part + (int64_t)blockIdx.x * VW_PART;
#pragma unroll
    for (int k = 0; k < 32; k++)
        out[j * 64 + c0 + k] = a10[k];
    const int t0 = tid < 128 ? 0 : 5, nt = tid < 128 ? 5 : 4;
#pragma unroll
    for (int k = 0; k < 5; k++)
        if (k < nt)
            out[128 * 64 + c * 9 + t0 + k] = a9[k];
}

// every head gradient = the sum of its workgroups' partial sums in workgroup order; loss = sum of squares / n_mean
__global__ __launch_bounds__(256) void value_head_reduce_kernel(const float *wpart, const float *hpart, int n_parts,
                                                                float n_mean, float *dw10, float *dw9, float *dw11,
                                                                float *db9, float *loss)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= VW_PART + VHEAD_PART)
        return;
    const bool w = t < VW_PART;
    const float *src = w ? wpart + t : hpart + (t - VW_PART);
    const int stride = w ? VW_PART : VHEAD_PART;
    float s = 0.0f;
    for (int g = 0; g < n_parts; g++)
        s += src[(int64_t)g * stride];
    if (t < 128 * 64)
        dw10[t] = s;
    else if (t < VW_PART)
        dw9[t - 128 * 64] = s;
    else if (t < VW_PART + 128)
        dw11[t - VW_PART] = s;
    else if (t == VW_PART + 128)
        *db9 = s;
    else
        *loss = s / n_mean;
}

// ---- The weight and bias gradients of block 1 (3x3, 2 -> 64 on the planes of the board: plane 0 = the opponent's
// stones, plane 1 = the mover's, game.py:168-174): dW1[co][plane][ky][kx] = sum over boards and cells of dY1[co][y][x]
// [plane has a stone at (y + ky - 1, x + kx - 1)], db1[co] = sum dY1.  One wave per board at a time, lane = channel.
constexpr int STEM_PART = 64 * 19;
__global__ __launch_bounds__(256) void stem_wgrad_kernel(const float *dy, const uint64_t *own, const uint64_t *opp, int64_t n,
                                                         float *part)
{
    __shared__ float red[4][STEM_PART];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float acc[19];
#pragma unroll
    for (int k = 0; k < 19; k++)
        acc[k] = 0.0f;
    for (int64_t b = (int64_t)blockIdx.x * 4 + wv; b < n; b += (int64_t)gridDim.x * 4) {
        const uint64_t pl[2] = {opp[b], own[b]};
        const float *src = dy + ((b * 4 + (lane >> 4)) * 64) * 16 + (lane & 15);
        for (int cell = 0; cell < 64; cell++) {
            const float d = src[cell * 16];
            const int y = cell >> 3, x = cell & 7;
            acc[18] += d;
#pragma unroll
            for (int ky = 0; ky < 3; ky++)
#pragma unroll
                for (int kx = 0; kx < 3; kx++) {
                    const int yy = y + ky - 1, xx = x + kx - 1;
                    const bool in = yy >= 0 && yy < 8 && xx >= 0 && xx < 8;
                    const int bit = in ? yy * 8 + xx : 0;
#pragma unroll
                    for (int pn = 0; pn < 2; pn++)
                        if (in && ((pl[pn] >> bit) & 1ull))
                            acc[pn * 9 + ky * 3 + kx] += d;
                }
        }
    }
#pragma unroll
    for (int k = 0; k < 19; k++)
        red[wv][lane * 19 + k] = acc[k];
    __syncthreads();
    for (int j = threadIdx.x; j < STEM_PART; j += 256)
        part[(int64_t)blockIdx.x * STEM_PART + j] = red[0][j] + red[1][j] + red[2][j] + red[3][j];
}

__global__ __launch_bounds__(256) void stem_reduce_kernel(const float *part, int n_parts, float *dw1, float *db1)
{
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63; // (channel, 18 weights + 1 bias)
    if (j >= STEM_PART)
        return;
    float s = 0.0f;
    for (int i = lane; i < n_parts; i += 64)
        s += part[(int64_t)i * STEM_PART + j];
    s = wave_sum(s);
    if (lane != 0)
        return;
    const int co = j / 19, k = j - 19 * co;
    if (k < 18)
        dw1[co * 18 + k] = s;
    else
        db1[co] = s;
}


// ---- chainer.optimizers.Adam + the WeightDecay hook (src/train_rl.py:24-26,66) over all parameters in one launch: the
// documented rule operation by operation, each product, sum, root and quotient rounded on its own (no fused
// multiply-adds), i.e. the bits of the elementwise float32 restatement in iago_amd/train_rl.py
struct AdamParams {
    float *p[IAGO_ADAM_MAX_TENSORS];
    const float *g[IAGO_ADAM_MAX_TENSORS];
    float *m[IAGO_ADAM_MAX_TENSORS], *v[IAGO_ADAM_MAX_TENSORS], *step[IAGO_ADAM_MAX_TENSORS];
    int64_t end[IAGO_ADAM_MAX_TENSORS]; // running element counts
    int32_t n_tensors;
    float alpha_t, one_minus_beta1, one_minus_beta2, eps, weight_decay;
};

__global__ __launch_bounds__(256) void adam_chainer_kernel(AdamParams A)
{
#pragma clang fp contract(off) // (a product and the sum behind it must not fuse)
    const int64_t total = A.end[A.n_tensors - 1];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        int s = 0;
        while (i >= A.end[s])
            s++;
        const int64_t j = i - (s ? A.end[s - 1] : 0);
        const float p = A.p[s][j], m = A.m[s][j], v = A.v[s][j];
        // (plain operators: the pragma above covers THIS function's expressions, not those inside HIP's __f*_rn inlines)
        const float wd_p = p * A.weight_decay;
        const float g = A.g[s][j] + wd_p;                        // the hook: g += rate * w
        const float dm = g - m;
        const float dm2 = dm * A.one_minus_beta1;
        const float m2 = m + dm2;                                // m += (1 - beta1)(g - m)
        const float gg = g * g;
        const float dv = gg - v;
        const float dv2 = dv * A.one_minus_beta2;
        const float v2 = v + dv2;                                // v += (1 - beta2)(g g - v)
        const float root = sqrtf(v2); // (correctly rounded; HIP's __fsqrt_rn is the native approximation)
        const float den = root + A.eps;
        A.m[s][j] = m2;
        A.v[s][j] = v2;
        const float num = m2 * A.alpha_t;
        const float step = num / den;                            // alpha_t m / (sqrt(v) + eps)
        if (A.step[s])
            A.step[s][j] = step; // (the caller subtracts it: its tensor library then knows the parameter changed)
        else
            A.p[s][j] = p - step;
    }
}

} // namespace

extern "C" {

int iago_conv3x3_wgrad_split(const void *dy_hi, const void *dy_lo, const void *x_hi, const void *x_lo, int64_t n,
                             int32_t cin, float *part, int32_t groups, const int32_t *scale_exp, float *dw, void *stream)
{
    if (n < 0 || (cin != 64 && cin != 128) || groups < 8 || (groups % 8) != 0)
        return iago_fail(IAGO_ERR_INVALID, "iago_conv3x3_wgrad_split: cin must be 64 or 128, groups a multiple of 8");
    if (!dy_hi || !dy_lo || !x_hi || !x_lo || !part)
        return iago_fail(IAGO_ERR_INVALID, "iago_conv3x3_wgrad_split: null pointer");
    static std::atomic<uint64_t> configured{0};
    if (iago_reserve_lds((const void *)wgrad_split_kernel, WG_LDS, configured,
                         "iago_conv3x3_wgrad_split: cannot reserve 78 KB of LDS"))
        return IAGO_ERR_HIP;
    WgradParams P;
    P.dy_hi = (const u32x4 *)dy_hi;
    P.dy_lo = (const u32x4 *)dy_lo;
    P.x_hi = (const u32x4 *)x_hi;
    P.x_lo = (const u32x4 *)x_lo;
    P.part = part;
    P.n = n;
    P.cin = cin;
    P.groups = groups;
    const unsigned grid = (unsigned)(groups * 2 * (cin / 32));
    hipLaunchKernelGGL(wgrad_split_kernel, dim3(grid), dim3(256), WG_LDS, (hipStream_t)stream, P);
    const int total = 9 * 128 * cin;
    if (dw) // (NULL: the partial sums only -- iago_policy_reinforce_grad reduces those of all blocks in one launch)
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           (const float *)part, groups, cin, scale_exp, dw);
    return iago_check_launch("iago_conv3x3_wgrad_split");
}


static int64_t pg_round(int64_t b)
{
    return (b + 255) & ~(int64_t)255;
}
constexpr int PG_GRID = 256;        // workgroups of the head and block-1 kernels (grid-stride over the boards: any device)
constexpr int PG_MAX_GROUPS = 64;

// groups of boards of a weight-gradient launch: one workgroup per CU (groups x 2 x cin / 32 workgroups), a multiple of 8
// (the workgroups of a group share an XCD), at most PG_MAX_GROUPS (the partial sums' scratch)
static int pg_groups(int cin)
{
    // (asked of the runtime once per device, as iago_mcts_search_capacity does: a process may drive devices of
    // different sizes, and the partial sums' grouping -- hence the gradients' last bits -- follows the device)
    static std::atomic<int> known[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess)
        dev = 0;
    int n = known[dev & 63].load(std::memory_order_acquire);
    if (n == 0) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v < 1)
            v = 256;
        known[dev & 63].store(v, std::memory_order_release);
        n = v;
    }
    int g = n / (2 * (cin / 32)) / 8 * 8;
    return g < 8 ? 8 : g > PG_MAX_GROUPS ? PG_MAX_GROUPS : g;
}

int64_t iago_policy_grad_workspace_bytes(int64_t n)
{
    if (n < 0)
        return -1;
    int64_t b = 0;
    b += 2 * pg_round(n * 8192) + 14 * pg_round(n * 16384);          // saved activations of blocks 1..8, hi + lo
    b += pg_round(n * 32768) + 2 * pg_round(n * 16384);              // a gradient as float32 and as scaled pieces
    b += 6 * pg_round((int64_t)PG_MAX_GROUPS * 9 * 128 * 128 * 4) +
         pg_round((int64_t)PG_MAX_GROUPS * 9 * 128 * 64 * 4);        // partial weight gradients, a buffer per block
    b += 7 * pg_round(((n * 8 + 1) / 2) * 32 * 4);                   // partial bias gradients, a buffer per block
    b += pg_round((int64_t)PG_GRID * HEAD_PART * 4) + pg_round((int64_t)PG_GRID * STEM_PART * 4);
    b += 256;                                                        // the tensors' largest magnitudes and scales
    return b;
}

extern "C++" { // (a template: C++ linkage inside the C entry points' block)

// What the trunk of both nets' updates reads and writes (blocks 1..8: SLPolicy and Value share their shape)
struct PgTrunk {
    const uint64_t *own, *opp;
    int64_t n;
    const float *w1, *b1;
    const void *const *w_hi, *const *w_lo, *const *wt_hi, *const *wt_lo;
    const float *const *bias;
    float *g_w1, *g_b1;
    float *const *g_w, *const *g_b;
    uint32_t *overflow;
};
// the trunk's scratch, carved from the front of the workspace (iago_policy_grad_workspace_bytes)
struct PgScratch {
    void *x_hi[8], *x_lo[8];
    float *dyf;
    void *dys_hi, *dys_lo;
    float *wpart[7], *bpart[7], *hpart, *spart;
    uint32_t *max_bits; // [0..7]: of the gradient at block k + 1's pre-activations; [16..23]: scales
    int32_t *scale_exp;
    char *end;          // the first byte after the trunk's scratch
};

// Forward with every block's output kept, head(S) -- which leaves the float32 gradient at block 8's pre-activations
// in S.dyf and raises S.max_bits[7] --, then blocks 8 .. 2, the one reduction launch, block 1
template <class Head>
static int pg_trunk_grad(const PgTrunk &T, void *workspace, void *stream, const char *who, Head head)
{
    const int64_t n = T.n;
    hipStream_t st = (hipStream_t)stream;
    PgScratch S;
    char *at = (char *)workspace;
    auto take = [&](int64_t bytes) {
        char *p = at;
        at += pg_round(bytes);
        return (void *)p;
    };
    for (int k = 0; k < 8; k++) {
        S.x_hi[k] = take(n * (k ? 16384 : 8192));
        S.x_lo[k] = take(n * (k ? 16384 : 8192));
    }
    S.dyf = (float *)take(n * 32768);
    S.dys_hi = take(n * 16384);
    S.dys_lo = take(n * 16384);
    // (partial sums of the weight and bias gradients: a buffer per block, reduced by ONE launch at the end)
    for (int k = 0; k < 7; k++) {
        S.wpart[k] = (float *)take((int64_t)PG_MAX_GROUPS * 9 * 128 * (k ? 128 : 64) * 4);
        S.bpart[k] = (float *)take(((n * 8 + 1) / 2) * 32 * 4);
    }
    S.hpart = (float *)take((int64_t)PG_GRID * HEAD_PART * 4);
    S.spart = (float *)take((int64_t)PG_GRID * STEM_PART * 4);
    S.max_bits = (uint32_t *)take(256);
    S.scale_exp = (int32_t *)(S.max_bits + 16);
    S.end = at;
    if (hipMemsetAsync(S.max_bits, 0, 256, st) != hipSuccess)
        return iago_fail(IAGO_ERR_HIP, (std::string(who) + ": hipMemsetAsync failed").c_str());

    // forward, every block's output kept
    int rc = iago_value_stem_boards(T.own, T.opp, T.w1, T.b1, S.x_hi[0], S.x_lo[0], n, T.overflow, stream);
    for (int k = 0; k < 7 && rc == IAGO_OK; k++)
        rc = iago_conv3x3_split(S.x_hi[k], S.x_lo[k], T.w_hi[k], T.w_lo[k], T.bias[k], S.x_hi[k + 1], S.x_lo[k + 1], n,
                                k ? 128 : 64, 128, T.overflow, stream);
    if (rc != IAGO_OK)
        return rc;
    rc = head(S);
    // blocks 8 .. 2: the gradient at the block's pre-activations (float32 in dyf) -> its scaled pieces + the bias
    // gradient; the weight gradient; the gradient at the pre-activations of the block below
    for (int k = 6; k >= 0 && rc == IAGO_OK; k--) {
        const int cin = k ? 128 : 64;
        rc = iago_split_scaled(S.dyf, S.max_bits + k + 1, S.dys_hi, S.dys_lo, S.scale_exp + k + 1, n, 128, S.bpart[k],
                               nullptr, stream);
        if (rc == IAGO_OK)
            rc = iago_conv3x3_wgrad_split(S.dys_hi, S.dys_lo, S.x_hi[k], S.x_lo[k], n, cin, S.wpart[k], pg_groups(cin),
                                          S.scale_exp + k + 1, nullptr, stream);
        if (rc == IAGO_OK)
            rc = iago_conv3x3_bwd_data_split(S.dys_hi, S.dys_lo, S.scale_exp + k + 1, T.wt_hi[k], T.wt_lo[k], S.x_hi[k],
                                             S.x_lo[k], cin, S.dyf, S.max_bits + k, n, stream);
    }
    if (rc != IAGO_OK)
        return rc;
    {
        ReduceAllParams Rp;
        int at_block = 0;
        for (int k = 0; k < 7; k++) {
            const int cin = k ? 128 : 64;
            Rp.wpart[k] = S.wpart[k];
            Rp.bpart[k] = S.bpart[k];
            Rp.dw[k] = T.g_w[k];
            Rp.db[k] = T.g_b[k];
            Rp.scale_exp[k] = S.scale_exp + k + 1;
            Rp.groups[k] = pg_groups(cin);
            Rp.cin[k] = cin;
            Rp.w_block0[k] = at_block;
            at_block += (9 * 128 * cin + 255) / 256;
        }
        Rp.w_block0[7] = at_block;
        Rp.n = n;
        hipLaunchKernelGGL(grad_reduce_all_kernel, dim3((unsigned)(at_block + 7 * 128 / 4)), dim3(256), 0, st, Rp);
    }
    // block 1 from the float32 gradient at its pre-activations
    hipLaunchKernelGGL(stem_wgrad_kernel, dim3(PG_GRID), dim3(256), 0, st, (const float *)S.dyf, T.own, T.opp, n, S.spart);
    hipLaunchKernelGGL(stem_reduce_kernel, dim3((STEM_PART + 3) / 4), dim3(256), 0, st, (const float *)S.spart, PG_GRID,
                       T.g_w1, T.g_b1);
    return iago_check_launch(who);
}

} // extern "C++"

int iago_policy_reinforce_grad(const iago_policy_grad_args *A, void *stream)
{
    if (!A || A->n < 0 || A->n_mean <= 0)
        return iago_fail(IAGO_ERR_INVALID, "iago_policy_reinforce_grad: bad arguments");
    const int64_t n = A->n;
    if (!A->own || !A->opp || !A->action || !A->reward || !A->w1 || !A->b1 || !A->w9 || !A->b10 || !A->g_w1 ||
        !A->g_b1 || !A->g_w9 || !A->g_b10 || !A->loss || !A->workspace)
        return iago_fail(IAGO_ERR_INVALID, "iago_policy_reinforce_grad: null pointer");
    for (int k = 0; k < 7; k++)
        if (!A->w_hi[k] || !A->w_lo[k] || !A->wt_hi[k] || !A->wt_lo[k] || !A->bias[k] || !A->g_w[k] || !A->g_b[k])
            return iago_fail(IAGO_ERR_INVALID, "iago_policy_reinforce_grad: null pointer (blocks 2..8)");
    if (A->workspace_bytes < iago_policy_grad_workspace_bytes(n) || ((uintptr_t)A->workspace & 255))
        return iago_fail(IAGO_ERR_INVALID, "iago_policy_reinforce_grad: workspace too small or not 256-byte aligned "
                                           "(iago_policy_grad_workspace_bytes)");
    if (n == 0)
        return iago_fail(IAGO_ERR_INVALID, "iago_policy_reinforce_grad: no rows");
    const PgTrunk T = {A->own, A->opp, n, A->w1, A->b1, A->w_hi, A->w_lo, A->wt_hi, A->wt_lo, A->bias,
                       A->g_w1, A->g_b1, A->g_w, A->g_b, A->overflow};
    // head + loss, forward and backward (src/train_rl.py:61-65)
    auto head = [&](const PgScratch &S) {
        hipStream_t st = (hipStream_t)stream;
        const float inv_n = 1.0f / (float)A->n_mean;
        HeadGradParams H;
        H.x_hi = (const uint4 *)S.x_hi[7];
        H.x_lo = (const uint4 *)S.x_lo[7];
        H.w9 = A->w9;
        H.b10 = A->b10;
        H.action = A->action;
        H.reward = A->reward;
        H.inv_n = inv_n;
        H.n = n;
        H.dy = (float4v *)S.dyf;
        H.max_bits = S.max_bits + 7;
        H.part = S.hpart;
        H.probs = A->probs;
        H.bad = A->overflow;
        hipLaunchKernelGGL(head_grad_kernel, dim3(PG_GRID), dim3(256), 0, st, H);
        hipLaunchKernelGGL(head_reduce_kernel, dim3((HEAD_PART + 3) / 4), dim3(256), 0, st, (const float *)S.hpart,
                           PG_GRID, inv_n, A->g_w9, A->g_b10, A->loss);
        return IAGO_OK;
    };
    return pg_trunk_grad(T, A->workspace, stream, "iago_policy_reinforce_grad", head);
}

int iago_policy_visits_grad(const iago_policy_visits_grad_args *A, void *stream)
{
    if (!A)
        return iago_fail(IAGO_ERR_INVALID, "iago_policy_visits_grad: null arguments");
    const int64_t n = A->n;
    if (n <= 0 || A->n_mean <= 0)
        return iago_fail(IAGO_ERR_INVALID, "iago_policy_visits_grad: n and n_mean must be positive");
    if (!A->own || !A->opp || !A->visits || !A->w1 || !A->b1 || !A->w9 || !A->b10 || !A->g_w1 || !A->g_b1 ||
        !A->g_w9 || !A->g_b10 || !A->loss || !A->workspace)
        return iago_fail(IAGO_ERR_INVALID, "iago_policy_visits_grad: null pointer");
    for (int k = 0; k < 7; k++)
        if (!A->w_hi[k] || !A->w_lo[k] || !A->wt_hi[k] || !A->wt_lo[k] || !A->bias[k] || !A->g_w[k] || !A->g_b[k])
            return iago_fail(IAGO_ERR_INVALID, "iago_policy_visits_grad: null pointer (blocks 2..8)");
    if (A->workspace_bytes < iago_policy_grad_workspace_bytes(n) || ((uintptr_t)A->workspace & 255))
        return iago_fail(IAGO_ERR_INVALID, "iago_policy_visits_grad: workspace too small or not 256-byte aligned "
                                           "(iago_policy_grad_workspace_bytes)");
    const PgTrunk T = {A->own, A->opp, n, A->w1, A->b1, A->w_hi, A->w_lo, A->wt_hi, A->wt_lo, A->bias,
                       A->g_w1, A->g_b1, A->g_w, A->g_b, A->overflow};
    // head + loss, forward and backward: the cross-entropy against the rows' visit distributions
    auto head = [&](const PgScratch &S) {
        hipStream_t st = (hipStream_t)stream;
        const float inv_n = 1.0f / (float)A->n_mean;
        HeadVisitsGradParams H;
        H.x_hi = (const uint4 *)S.x_hi[7];
        H.x_lo = (const uint4 *)S.x_lo[7];
        H.w9 = A->w9;
        H.b10 = A->b10;
        H.visits = A->visits;
        H.weight = A->weight;
        H.inv_n = inv_n;
        H.n = n;
        H.dy = (float4v *)S.dyf;
        H.max_bits = S.max_bits + 7;
        H.part = S.hpart;
        H.probs = A->probs;
        H.bad = A->overflow;
        hipLaunchKernelGGL(head_visits_grad_kernel, dim3(PG_GRID), dim3(256), 0, st, H);
        hipLaunchKernelGGL(head_reduce_kernel, dim3((HEAD_PART + 3) / 4), dim3(256), 0, st, (const float *)S.hpart,
                           PG_GRID, inv_n, A->g_w9, A->g_b10, A->loss);
        return IAGO_OK;
    };
    return pg_trunk_grad(T, A->workspace, stream, "iago_policy_visits_grad", head);
}

// the head's scratch behind the trunk's: h9, dh10, dpre9 per board, the two head kernels' partial sums
static int64_t value_head_bytes(int64_t n)
{
    return 2 * pg_round(n * 64 * 4) + pg_round(n * 128 * 4) + pg_round((int64_t)PG_GRID * VHEAD_PART * 4) +
           pg_round((int64_t)PG_GRID * VW_PART * 4);
}

int64_t iago_value_grad_workspace_bytes(int64_t n)
{
    if (n < 0)
        return -1;
    return iago_policy_grad_workspace_bytes(n) + value_head_bytes(n);
}

int iago_value_mse_grad(const iago_value_grad_args *A, void *stream)
{
    if (!A)
        return iago_fail(IAGO_ERR_INVALID, "iago_value_mse_grad: null arguments");
    const int64_t n = A->n;
    if (n <= 0 || A->n_mean <= 0)
        return iago_fail(IAGO_ERR_INVALID, "iago_value_mse_grad: n and n_mean must be positive");
    if (!A->own || !A->opp || !A->result || !A->w1 || !A->b1 || !A->w9 || !A->b9 || !A->w10 || !A->w11 ||
        !A->g_w1 || !A->g_b1 || !A->g_w9 || !A->g_b9 || !A->g_w10 || !A->g_w11 || !A->loss || !A->workspace)
        return iago_fail(IAGO_ERR_INVALID, "iago_value_mse_grad: null pointer");
    for (int k = 0; k < 7; k++)
        if (!A->w_hi[k] || !A->w_lo[k] || !A->wt_hi[k] || !A->wt_lo[k] || !A->bias[k] || !A->g_w[k] || !A->g_b[k])
            return iago_fail(IAGO_ERR_INVALID, "iago_value_mse_grad: null pointer (blocks 2..8)");
    if (A->workspace_bytes < iago_value_grad_workspace_bytes(n) || ((uintptr_t)A->workspace & 255))
        return iago_fail(IAGO_ERR_INVALID, "iago_value_mse_grad: workspace too small or not 256-byte aligned "
                                           "(iago_value_grad_workspace_bytes)");
    if (!isfinite(A->dropout_scale))
        return iago_fail(IAGO_ERR_INVALID, "iago_value_mse_grad: dropout_scale must be finite");
    const PgTrunk T = {A->own, A->opp, n, A->w1, A->b1, A->w_hi, A->w_lo, A->wt_hi, A->wt_lo, A->bias,
                       A->g_w1, A->g_b1, A->g_w, A->g_b, A->overflow};
    // head + loss, forward and backward (train_value.py:53-57)
    auto head = [&](const PgScratch &S) {
        hipStream_t st = (hipStream_t)stream;
        char *at = S.end;
        auto take = [&](int64_t bytes) {
            char *p = at;
            at += pg_round(bytes);
            return (float *)p;
        };
        float *h9 = take(n * 64 * 4), *dh10 = take(n * 128 * 4), *dpre9 = take(n * 64 * 4);
        float *hpart = take((int64_t)PG_GRID * VHEAD_PART * 4), *wpart = take((int64_t)PG_GRID * VW_PART * 4);
        ValueHeadGradParams H;
        H.x_hi = (const uint4 *)S.x_hi[7];
        H.x_lo = (const uint4 *)S.x_lo[7];
        H.w9 = A->w9;
        H.b9 = A->b9;
        H.w10 = A->w10;
        H.w11 = A->w11;
        H.result = A->result;
        H.keep = A->keep;
        H.scale = A->dropout_scale;
        H.two_over_n = (float)(2.0 / (double)A->n_mean); // (Chainer: gy * float32(2 / size))
        H.n = n;
        H.dy = (float4v *)S.dyf;
        H.max_bits = S.max_bits + 7;
        H.h9 = h9;
        H.dh10 = dh10;
        H.dpre9 = dpre9;
        H.part = hpart;
        H.pred = A->pred;
        H.h9_out = A->h9;
        hipLaunchKernelGGL(value_head_grad_kernel, dim3(PG_GRID), dim3(256), 0, st, H);
        ValueWgradParams W;
        W.x_hi = (const uint4 *)S.x_hi[7];
        W.x_lo = (const uint4 *)S.x_lo[7];
        W.h9 = h9;
        W.dh10 = dh10;
        W.dpre9 = dpre9;
        W.n = n;
        W.part = wpart;
        hipLaunchKernelGGL(value_head_wgrad_kernel, dim3(PG_GRID), dim3(256), 0, st, W);
        hipLaunchKernelGGL(value_head_reduce_kernel, dim3((VW_PART + VHEAD_PART + 255) / 256), dim3(256), 0, st,
                           (const float *)wpart, (const float *)hpart, PG_GRID, (float)A->n_mean, A->g_w10, A->g_w9,
                           A->g_w11, A->g_b9, A->loss);
        return IAGO_OK;
    };
    return pg_trunk_grad(T, A->workspace, stream, "iago_value_mse_grad", head);
}

int iago_adam_chainer(const iago_adam_args *a, void *stream)
{
    if (!a || a->n_tensors < 1 || a->n_tensors > IAGO_ADAM_MAX_TENSORS)
        return iago_fail(IAGO_ERR_INVALID, "iago_adam_chainer: 1 .. IAGO_ADAM_MAX_TENSORS tensors expected");
    AdamParams A;
    int64_t total = 0;
    for (int k = 0; k < a->n_tensors; k++) {
        if (!a->p[k] || !a->g[k] || !a->m[k] || !a->v[k] || a->count[k] <= 0)
            return iago_fail(IAGO_ERR_INVALID, "iago_adam_chainer: null pointer or empty tensor");
        A.p[k] = a->p[k];
        A.g[k] = a->g[k];
        A.m[k] = a->m[k];
        A.v[k] = a->v[k];
        A.step[k] = a->step[k];
        total += a->count[k];
        A.end[k] = total;
    }
    A.n_tensors = a->n_tensors;
    A.alpha_t = a->alpha_t;
    A.one_minus_beta1 = a->one_minus_beta1;
    A.one_minus_beta2 = a->one_minus_beta2;
    A.eps = a->eps;
    A.weight_decay = a->weight_decay;
    const int64_t blocks = (total + 255) / 256;
    hipLaunchKernelGGL(adam_chainer_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0,
                       (hipStream_t)stream, A);
    return iago_check_launch("iago_adam_chainer");
}

} // extern "C"
