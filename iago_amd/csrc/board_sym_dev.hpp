// board_sym_dev.hpp -- the board's symmetries on a bitboard and on a cell index (bit a = row*8+col): the two generators
// of iago_augment8's eight variants (rules_kernels.hip) and of iago_replay_sample's (replay_kernels.hip), and the
// canonical form of a position under them (iago_canonical_rows, iago_replay_merge).
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace iago {

__device__ __forceinline__ uint64_t bb_transpose(uint64_t x) // (y,x) -> (x,y)
{
    uint64_t t = (x ^ (x >> 7)) & 0x00AA00AA00AA00AAull;
    x ^= t ^ (t << 7);
    t = (x ^ (x >> 14)) & 0x0000CCCC0000CCCCull;
    x ^= t ^ (t << 14);
    t = (x ^ (x >> 28)) & 0x00000000F0F0F0F0ull;
    x ^= t ^ (t << 28);
    return x;
}
// np.rot90 (counter-clockwise): (y,x) -> (7-x, y) = transpose, then flip the rows
__device__ __forceinline__ uint64_t bb_rot90(uint64_t x) { return __builtin_bswap64(bb_transpose(x)); }
__device__ __forceinline__ int act_rot90(int a) { return a < 0 ? a : (7 - (a & 7)) * 8 + (a >> 3); }
__device__ __forceinline__ int act_transpose(int a) { return a < 0 ? a : (a & 7) * 8 + (a >> 3); }

// The eight variants in iago_augment8's order (load.py:56-74): 0 the identity, 1 .. 3 successive quarter turns, 4 the
// transpose of variant 3, 5 .. 7 three more turns -- step i of the chain is a transpose for i == 4, a turn otherwise.
__device__ __forceinline__ uint64_t bb_variant(uint64_t x, int k)
{
    for (int i = 1; i <= k; i++)
        x = (i == 4) ? bb_transpose(x) : bb_rot90(x);
    return x;
}
__device__ __forceinline__ int act_variant(int a, int k) // m_k(a); a < 0 stays
{
    for (int i = 1; i <= k; i++)
        a = (i == 4) ? act_transpose(a) : act_rot90(a);
    return a;
}
// The cell a with m_k(a) == d: four turns are the identity and the transpose undoes itself, so the inverse of k < 4
// turns is 4 - k turns, and that of m_k = turn^(k-4) . transpose . turn^3 is turn . transpose . turn^(8-k).
__device__ __forceinline__ int act_variant_inverse(int d, int k)
{
    const int turns = (k < 4 ? 4 - k : 8 - k) & 3;
    for (int i = 0; i < turns; i++)
        d = act_rot90(d);
    return k < 4 ? d : act_rot90(act_transpose(d));
}

// The canonical form of a position (iago_canonical_rows): of the eight pairs (bb_variant(own, k), bb_variant(opp, k))
// the smallest, own compared first, then opp, both as unsigned 64-bit; returns the lowest k that gives it and leaves
// that pair in own / opp.  The chain of bb_variant walked once: a strict "smaller" keeps the lowest k of a tie.
__device__ __forceinline__ int bb_canonical(uint64_t &own, uint64_t &opp)
{
    uint64_t o = own, p = opp, best_o = own, best_p = opp;
    int best = 0;
    for (int k = 1; k < 8; k++) {
        o = (k == 4) ? bb_transpose(o) : bb_rot90(o);
        p = (k == 4) ? bb_transpose(p) : bb_rot90(p);
        if (o < best_o || (o == best_o && p < best_p)) {
            best_o = o;
            best_p = p;
            best = k;
        }
    }
    own = best_o;
    opp = best_p;
    return best;
}
// act_variant_inverse(d, k) for all eight k at once, byte k of the result: a lane that turns many rows by varying k
// picks its source cell with one shift (a register array indexed by k would go to scratch).
__device__ __forceinline__ uint64_t act_variant_inverse_all(int d)
{
    uint64_t packed = 0ull;
    for (int k = 0; k < 8; k++)
        packed |= (uint64_t)act_variant_inverse(d, k) << (8 * k);
    return packed;
}

} // namespace iago
