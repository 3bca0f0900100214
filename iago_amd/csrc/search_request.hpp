// search_request.hpp -- the persistent search's request and reply, stated once (search_kernel.hip: the rings, the
// mailboxes; conv_trunk_body.hpp / conv_policy_body.hpp: the walks read the position out of a request's LDS copy).
//
// A request is WORDS 32-bit words.  In a ring it is entry `t` (ticket t): WORDS granules of 8 bytes in a slot of
// SLOT_STRIDE granules, granule i = entry_word(t, word i) -- the ticket's tag in the high half, so that the data is
// the flag.  A net workgroup keeps the low halves, WORDS words per request, in LDS: what the accessors below read.
// A reply is one granule per value (or 64 per distribution): reply_word(the request's reply tag, the float's bits).
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace iago_request {

enum Word {
    W_WHO = 0,   // kind bit (bit 31) | game: the slot whose mailbox takes the reply, or NOBODY
    W_TAG,       // the reply's tag (the game's epoch; a NOBODY request: the sender, for the table's writer field)
    W_OWN_LO, W_OWN_HI, // the position: own = the side to move
    W_OPP_LO, W_OPP_HI,
    WORDS
};
constexpr int SLOT_STRIDE = 8;            // granules between two entries of a ring (WORDS in use)
constexpr uint32_t NOBODY = 0x7FFFFFFFu;  // "game" of a request nobody waits for (its value goes to the position table only)
constexpr uint32_t KIND_VALUE = 0u, KIND_POLICY = 1u; // (the ring, too: one ring per kind)

__host__ __device__ __forceinline__ uint32_t who_word(uint32_t kind, uint32_t game) { return (kind << 31) | game; }
__host__ __device__ __forceinline__ uint32_t kind(const uint32_t *r) { return r[W_WHO] >> 31; }
__host__ __device__ __forceinline__ uint32_t game(const uint32_t *r) { return r[W_WHO] & 0x7FFFFFFFu; }
__host__ __device__ __forceinline__ uint32_t tag(const uint32_t *r) { return r[W_TAG]; }
__host__ __device__ __forceinline__ uint64_t own(const uint32_t *r) { return ((uint64_t)r[W_OWN_HI] << 32) | r[W_OWN_LO]; }
__host__ __device__ __forceinline__ uint64_t opp(const uint32_t *r) { return ((uint64_t)r[W_OPP_HI] << 32) | r[W_OPP_LO]; }

// a ring's granule: ticket t's tag (t + 1: a zeroed ring holds nobody's entry) over one word of the request
__host__ __device__ __forceinline__ unsigned long long entry_word(uint32_t t, uint32_t x)
{
    return ((unsigned long long)(t + 1u) << 32) | x;
}
__host__ __device__ __forceinline__ bool entry_is(unsigned long long x, uint32_t t) { return (uint32_t)(x >> 32) == t + 1u; }

// a mailbox's granule
__host__ __device__ __forceinline__ unsigned long long reply_word(uint32_t tag, uint32_t bits)
{
    return ((unsigned long long)tag << 32) | bits;
}
__host__ __device__ __forceinline__ uint32_t reply_tag(unsigned long long x) { return (uint32_t)(x >> 32); }
__host__ __device__ __forceinline__ uint32_t reply_bits(unsigned long long x) { return (uint32_t)x; }

} // namespace iago_request
