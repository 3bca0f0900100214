// mcts_dev.hpp -- the tree arithmetic of MCTS.py, stated once for every search kernel: the per-playout kernels
// (mcts_kernels.hip) and the persistent, wave and park searches (search_kernel.hip) build bit-identical trees because they
// call these functions.  Node.select's score and its argmax butterfly, the stone of a selection, Node.expand, the leaf
// mix, the value cache, Node.update, a fresh root and the z-log record; what a schedule adds (where a prior is read,
// which lane writes, queues, paths) stays with its kernel.  puct_score and leaf_mix are compiled with floating-point
// contraction off: every product and sum is rounded on its own, as numpy rounds them.
#pragma once
#include "abi_common.hpp"
#include "othello_dev.hpp"
#include "../../include/iago_hip_serving.h" // (iago_root_noise)

#include <math.h>
#include <string>

namespace iago_mcts {
using namespace iago;

constexpr int BLOCK = 256;
constexpr int MAX_DEPTH = 512; // bound on the descent (a path adds a node per expansion)

typedef iago_mcts_tree Tree;

__device__ __forceinline__ void init_node(const Tree &T, int64_t i, int parent, int action, float p)
{
    T.nodes[i].parent = parent;
    T.nodes[i].first_child = -1;
    T.nodes[i].n_children = 0;
    T.nodes[i].action = (int8_t)action;
    T.nodes[i].n_visits = 0;
    T.nodes[i].q = 0.0f;
    T.nodes[i].p = p;
    T.nodes[i].reserved1 = 0; // in-flight visits of the wave search (search_kernel.hip): none
    if (T.has_v)
        T.nodes[i].v = __builtin_nanf(""); // value_func(node) not evaluated yet
}

// Node(None, 1.0) as game g's only node, its root (MCTS.py:81,154; one lane).  1.1 under either selection rule (below): a
// root's prior is never read
__device__ __forceinline__ void fresh_root(const Tree &T, int64_t g, int64_t base)
{
    init_node(T, base, -1, -2, 1.0f + 0.1f);
    T.n_nodes[g] = 1;
    T.root[g] = 0;
}

// the two halves of a node record: s = {n_visits, q, p, v}, l = {first_child, parent, action | n_children << 8, vv}
__device__ __forceinline__ void node_record(const Tree &T, int64_t at, uint4 &s, uint4 &l)
{
    s = ((const uint4 *)&T.nodes[at])[0];
    l = ((const uint4 *)&T.nodes[at])[1];
}

// ---- the selection rule ("Selection rule"; the contract is iago_hip_serving.h's, IAGO_SEARCH_PUCT_AZ): two
// constants, uniform over a launch.  prior_off is added to the prior a child stores (make_children), visit_off to the
// visits in the exploration term's denominator (puct_score, wave_score).  The reference's rule: 0.1f and 0.01 (MCTS.py:19,
// 49) -- the same operations on the same bits as the literals were, so its trees are what they always were.  The AlphaZero
// rule: 0.0f and 1.0 -- P = prob (x + 0.0f is x for the policy's positive outputs), U = c_puct P sqrt(N) / (1 + n).  A
// root made by fresh_root keeps 1.0f + 0.1f under both (its prior is never read).  The per-playout kernels
// (mcts_kernels.hip) pass the reference's pair
constexpr float PRIOR_OFF_REFERENCE = 0.1f, PRIOR_OFF_ALPHAZERO = 0.0f;
constexpr double VISIT_OFF_REFERENCE = 0.01, VISIT_OFF_ALPHAZERO = 1.0;

// ---- Node.select (MCTS.py:39-49)

// Node.get_value (MCTS.py:75-76) of a child with prior p, value q and n visits under a parent with sq =
// np.sqrt(parent.n_visits): float32 c_puct * P, float64 sqrt, divide and add, as numpy >= 2 promotes them (MCTS.py:49).
// visit_off: the rule's (above)
__device__ __forceinline__ double puct_score(float c_puct, float p, float q, int n, double sq, double visit_off)
{
#pragma clang fp contract(off)
    const float cp = c_puct * p;
    const double u = (double)cp * sq / (visit_off + (double)n);
    return (double)q + u;
}

// ---- forced playouts ("Forced playouts"; the contract is iago_hip_serving.h's): forced(n, p, N) of a
// root child with n visits and the STORED prior p under a root of N visits, k = k_256 / 256: n >= 1 and 256 n^2 < (k_256 p)
// N -- n < sqrt(k p N) without the root.  256 n^2 (n < 2^22) and k_256 p (12 x 24 bits) are exact in float64, the product
// with N rounds once; no contraction.  k_256 = 0: never
__device__ __forceinline__ bool forced_child(int n, float p, double k_256, double N)
{
#pragma clang fp contract(off)
    const double dn = (double)n;
    const double lhs = 256.0 * dn * dn;
    const double kp = k_256 * (double)p;
    const double rhs = kp * N;
    return n >= 1 && lhs < rhs;
}

// in-flight visits (vv) of a wave search: the score of a child when a playout of the wave is on its way through it --
// n + vv visits, the in-flight ones counted as a loss of `vloss` each.  vv == 0: puct_score exactly.  (No contraction:
// the restatement in tests/wave_mcts.py rounds every product and difference on its own)
__device__ __forceinline__ double wave_score(float c_puct, float p, float q, int n, int vv, double sq, double vloss,
                                             double visit_off)
{
#pragma clang fp contract(off)
    const float cp = c_puct * p;
    const int nc = n + vv;
    const double u = (double)cp * sq / (visit_off + (double)nc);
    const double qe = vv == 0 ? (double)q : ((double)q * (double)n - vloss * (double)vv) / (double)nc;
    return qe + u;
}

// the score of child j, whose record is (s, l), against the best of its lane so far; strict `>`: the first maximum wins
// (python max, MCTS.py:46).  pl: the best child's first_child, n_visits, action | n_children << 8 (| vv << 16), v
// FORCE (the noise instantiations of the persistent search alone): a child with forced_child(n, p, force_k, force_n) scores
// +inf -- the caller gives force_k = k_256 at the root of the search when it has two or more children, 0 anywhere else
template <bool WAVE, bool FORCE = false>
__device__ __forceinline__ void score_child(float c_puct, double vloss, double visit_off, uint4 s, uint4 l, int j, double sq,
                                            double &best_v, int &best_i, uint32_t (&pl)[4], double force_k = 0.0,
                                            double force_n = 0.0)
{
    const float p = __uint_as_float(s.z), q = __uint_as_float(s.y);
    const int n = (int)s.x;
    // (vv < 2^16: at most 32 playouts in flight)
    double v = WAVE ? wave_score(c_puct, p, q, n, (int)l.w, sq, vloss, visit_off) : puct_score(c_puct, p, q, n, sq, visit_off);
    if constexpr (FORCE)
        v = forced_child(n, p, force_k, force_n) ? (double)INFINITY : v;
    if (v > best_v) {
        best_v = v;
        best_i = j;
        pl[0] = l.x, pl[1] = (uint32_t)n, pl[2] = WAVE ? (l.z & 0xFFFFu) | (l.w << 16) : l.z & 0xFFFFu, pl[3] = s.w;
    }
}

// python's max over the children (MCTS.py:46) across the 8 lanes of a game: the larger score, of equal scores the
// smaller index -- every lane offers its first maximum, so the first maximum wins
template <int CTRL>
__device__ __forceinline__ void argmax_step(double &v, int &idx)
{
    const uint64_t bits = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = dpp_u32<CTRL>((uint32_t)bits), hi = dpp_u32<CTRL>((uint32_t)(bits >> 32));
    const double ov = __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
    const int oi = (int)dpp_u32<CTRL>((uint32_t)idx);
    const bool take = (ov > v) || (ov == v && oi < idx);
    v = take ? ov : v;
    idx = take ? oi : idx;
}

// the same step carrying four payload words of the winner
template <int CTRL>
__device__ __forceinline__ void argmax_step_payload(double &v, int &idx, uint32_t (&pl)[4])
{
    const uint64_t bits = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = dpp_u32<CTRL>((uint32_t)bits), hi = dpp_u32<CTRL>((uint32_t)(bits >> 32));
    const double ov = __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
    const int oi = (int)dpp_u32<CTRL>((uint32_t)idx);
    const bool take = (ov > v) || (ov == v && oi < idx);
    v = take ? ov : v;
    idx = take ? oi : idx;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t o = dpp_u32<CTRL>(pl[i]);
        pl[i] = take ? o : pl[i];
    }
}

// GameFunctions.place_stone(state, a, c); c = 3 - c (MCTS.py:131-132): move a (< 0: a pass, nothing placed) and the swap
// of sides.  Every lane of the group takes part (group8_flips)
__device__ __forceinline__ void place_stone(uint64_t &own, uint64_t &opp, int a, const Lane8 &L)
{
    const uint64_t f = group8_flips(to_lane(own, L), to_lane(opp, L), (uint32_t)a & 63u, L);
    uint64_t o = own, p = opp;
    if (a >= 0) {
        const uint64_t bit = 1ull << (a & 63);
        o = own | f | bit;
        p = opp & ~f & ~bit;
    }
    own = p;
    opp = o;
}

// ---- Node.expand (MCTS.py:27-37, 109-121), the 8 lanes of a game together

// k nodes of game g's pool, taken by the group's lane 0 (`lane0`; false on every lane: nothing is taken): first child + 1
// on every lane of the group, 0 = no room (reported in T.overflow) or nothing taken
__device__ __forceinline__ uint32_t alloc_children(const Tree &T, int64_t g, int k, bool lane0)
{
    uint32_t fc1 = 0;
    if (lane0) {
        const int at = T.n_nodes[g];
        if (at + k <= T.capacity) {
            T.n_nodes[g] = at + k;
            fc1 = (uint32_t)at + 1u;
        } else {
            T.overflow[g] = 1;
        }
    }
    return group8_add(fc1);
}

// the children of `node` for its legal moves lg, from pool index fc on.  No move (a pass child, action -1) or a single
// one: Node(node, 1.0) without a net (MCTS.py:112-117), by lane 0.  Else Node.expand (MCTS.py:27-37): lane r creates the
// children of board row r in ascending order of the move, child a with prior(a) + prior_off (MCTS.py:19: + 0.1; the
// selection rule's, above -- the lone child stores 1.0f + prior_off)
template <class Prior>
__device__ __forceinline__ void make_children(const Tree &T, int64_t base, int fc, int node, uint64_t lg, uint32_t r,
                                              float prior_off, Prior prior)
{
    if ((lg & (lg - 1ull)) == 0ull) {
        if (r == 0u)
            init_node(T, base + fc, node, lg ? (int)__builtin_ctzll(lg) : -1, 1.0f + prior_off);
    } else {
        uint32_t row = (uint32_t)(lg >> (8u * r)) & 0xFFu;
        int at = fc + __popcll(lg & ((1ull << (8u * r)) - 1ull));
        while (row) {
            const int a = (int)(8u * r) + __builtin_ctz(row);
            row &= row - 1u;
            init_node(T, base + at, node, a, prior(a) + prior_off);
            at++;
        }
    }
}

// the parent's side of an expansion (one lane)
__device__ __forceinline__ void link_children(const Tree &T, int64_t parent, int fc, int k)
{
    T.nodes[parent].first_child = fc;
    T.nodes[parent].n_children = (uint8_t)k;
}

// ---- the leaf's value (MCTS.py:123-125) and Node.update_recursive (MCTS.py:51-72)

// (1 - lmbda) * v + lmbda * z with numpy >= 2 scalar promotion (MCTS.py:123-125): the python-float factors are rounded to
// float32, products and sum in float32.  (v is not read at lmbda = 1, z not at lmbda = 0: MCTS.py:124-125 are skipped)
__device__ __forceinline__ float leaf_mix(float lmbda, float v, int8_t z)
{
#pragma clang fp contract(off)
    const float a = (lmbda < 1.0f) ? (float)(1.0 - (double)lmbda) * v : 0.0f;
    const float b = (lmbda > 0.0f) ? (float)((double)lmbda * (double)z) : 0.0f;
    return a + b;
}

// value_func(leaf) (MCTS.py:97-103,124) is a pure function of the leaf's position: with a value cache (T.v) the net runs
// only for the leaves it has not seen, whose fresh values vg are stored now (by the lanes with `writer`); the others
// take the stored value.  (Every lane of a game may read the slot while one writes it: the loads of a wave come before
// its stores)
__device__ __forceinline__ float cached_value(float *slot, float vg, bool writer)
{
    const float cached = *slot;
    if (cached == cached)
        return cached;
    if (writer)
        *slot = vg;
    return vg;
}

// Node.update (MCTS.py:58-63) with leaf value lv: (n_visits, Q) as one 8-byte load and one 8-byte store
__device__ __forceinline__ void visit(const Tree &T, int64_t at, float lv)
{
    uint2 *nq = (uint2 *)&T.nodes[at];
    const uint2 old = *nq;
    const int n = (int)old.x + 1;                // MCTS.py:61
    const float q = __uint_as_float(old.y);
    *nq = make_uint2((uint32_t)n, __float_as_uint(q + (lv - q) / (float)n)); // MCTS.py:63
}

// What visit() takes at index d of a playout's path of path_n nodes (0: the root, path_n - 1: the leaf), lv the leaf's value
// from the leaf mover's view.  The reference's rule (negamax == 0): lv at every level.  The negamax rule
// (IAGO_SEARCH_NEGAMAX; DESIGN.md section 7, "Backup rule"): a node's Q is the value for the player who moved INTO it, so
// the leaf takes -lv and the sign turns once per parent -- +lv where path_n - 1 - d is odd.  (-lv is exact)
// negamax is 0 or 1: the sign bit is turned by arithmetic (path_n - 1 - d even <=> path_n - d odd), not by a select whose
// lane mask the search kernels would have to keep
__device__ __forceinline__ float backup_value(int negamax, float lv, int path_n, int d)
{
    return __uint_as_float(__float_as_uint(lv) ^ (((uint32_t)(path_n - d) & (uint32_t)negamax) << 31));
}

// Node.update_recursive (MCTS.py:65-72) from `node` up to the root: the same value at every level, no sign flip
// (the per-playout launches keep the reference's rule)
__device__ __forceinline__ void backup_climb(const Tree &T, int64_t base, int node, float lv)
{
    for (int depth = 0; node >= 0 && depth <= MAX_DEPTH; depth++) {
        visit(T, base + node, lv);
        node = T.nodes[base + node].parent;
    }
}

// ---- exploring self-play ("Exploring self-play"): in the first explore_turns turns of a game the
// move is drawn in proportion to the root's visit counts n[a] (the children in ascending cell order), in integers:
// N = sum n, w = word turn & 3 of Philox4x32-10 on counter (game id, turn >> 2, 0, 0) under the rollouts' key with its
// high word XOR EXPLORE_KEY, r = (uint64(w) * N) >> 32, the move is the lowest cell a with sum_{b <= a} n[b] > r
// (N == 0: the most visited child's first-maximum rule stays)
constexpr uint32_t EXPLORE_KEY = 0x4558504Cu; // ("EXPL")
constexpr uint32_t CAP_KEY = 0x43415050u;     // ("CAPP": the playout cap, below)

// word turn & 3 of Philox4x32-10 on (id, turn >> 2, 0, 0) under (key0, key1)
__device__ __forceinline__ uint32_t turn_word(uint32_t key0, uint32_t key1, uint32_t id, uint32_t turn)
{
    uint32_t c[4] = {id, turn >> 2, 0u, 0u};
    philox4x32_10(c, key0, key1);
    const uint32_t lo = (turn & 1u) ? c[1] : c[0], hi = (turn & 1u) ? c[3] : c[2]; // (selects: no indexed array)
    return (turn & 2u) ? hi : lo;
}

__device__ __forceinline__ uint32_t explore_word(uint32_t key0, uint32_t key1, uint32_t id, uint32_t turn)
{
    return turn_word(key0, key1 ^ EXPLORE_KEY, id, turn);
}

// ---- playout-cap randomisation ("Playout cap"): a searched turn is FULL (n_sims playouts, a policy
// target) when the top byte of its word is below full_per_256, else FAST (the first n_fast playouts of the same search).
// The word is explore_word's -- word turn & 3 of Philox4x32-10 on (game id, turn >> 2, 0, 0) -- under a key of its own:
// the rollouts' key with its high word XOR CAP_KEY.  (The persistent search draws both words at ONE call site of turn_word,
// the key chosen per lane: a second Philox body cost it a register)
__device__ __forceinline__ uint32_t cap_word(uint32_t key0, uint32_t key1, uint32_t id, uint32_t turn)
{
    return turn_word(key0, key1 ^ CAP_KEY, id, turn);
}

__device__ __forceinline__ bool cap_fast_turn(uint32_t w, uint32_t full_per_256)
{
    return (w >> 24) >= full_per_256;
}

// the draw's threshold r in [0, total)
__device__ __forceinline__ uint32_t explore_threshold(uint32_t w, uint32_t total)
{
    return __umulhi(w, total);
}

// the draw across the 8 lanes of a game: row_n = the visit counts of this lane's 8 cells (8 l8 ..), 0 where no child.
// Every lane of the group takes part and receives the move; 64 when no child was visited
__device__ __forceinline__ int explore_draw8(const int (&row_n)[8], uint32_t l8, uint32_t w)
{
    uint32_t blk = 0u;
#pragma unroll
    for (int i = 0; i < 8; i++)
        blk += (uint32_t)row_n[i];
    // the sum over the group and the sum of the lower lanes (group8_scan's butterfly, in integers)
    uint32_t pre = 0u;
    uint32_t o = dpp_u32<DPP_XOR1>(blk);
    pre = (l8 & 1u) ? pre + o : pre;
    blk += o;
    o = dpp_u32<DPP_XOR2>(blk);
    pre = (l8 & 2u) ? pre + o : pre;
    blk += o;
    o = dpp_u32<DPP_HALF_MIRROR>(blk);
    pre = (l8 & 4u) ? pre + o : pre;
    blk += o;
    const uint32_t r = explore_threshold(w, blk);
    uint32_t a = 64u;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        pre += (uint32_t)row_n[i];
        a = (a == 64u && pre > r) ? 8u * l8 + (uint32_t)i : a;
    }
    // the lowest cell of the group (a lane whose lower lanes crossed r offers its first cell: a lower lane offers less)
    a = min(a, dpp_u32<DPP_XOR1>(a));
    a = min(a, dpp_u32<DPP_XOR2>(a));
    a = min(a, dpp_u32<DPP_HALF_MIRROR>(a));
    return blk == 0u ? 64 : (int)a;
}

// ---- root noise ("Root noise"; the contract is iago_hip_serving.h's): at a searched turn the priors
// of the root's K >= 2 children are mixed with the shares of a Polya urn over the mover's legal cells, in integers.  The
// urn: c[a] = 0; draw j = 0 .. N-1 takes the cell by explore_draw8's rule from the weights alpha_256 + 256 c[a] (their
// total is K alpha_256 + 256 j) with word j & 3 of Philox4x32-10 on (game id, turn, j >> 2, 0) under the rollouts' key
// with its high word XOR NOISE_KEY, and adds 1 to its c.  The counts are Dirichlet-multinomial(N, alpha_256 / 256).
constexpr uint32_t NOISE_KEY = IAGO_NOISE_KEY; // ("DIRI")

// (host) the noise's own arguments, for both entry points that take them
inline int check_root_noise(const iago_root_noise *nz, const char *who)
{
    const std::string w(who);
    if (!nz)
        return iago_fail(IAGO_ERR_INVALID, (w + ": null noise arguments").c_str());
    if (nz->reserved0 != 0)
        return iago_fail(IAGO_ERR_INVALID, (w + ": reserved fields must be 0").c_str());
    if (nz->alpha_256 < 1 || nz->alpha_256 > 4096)
        return iago_fail(IAGO_ERR_INVALID, (w + ": alpha_256 must be in [1, 4096]").c_str());
    if (nz->eps_256 < 0 || nz->eps_256 > 256)
        return iago_fail(IAGO_ERR_INVALID, (w + ": eps_256 must be in [0, 256]").c_str());
    if (nz->draws < 16 || nz->draws > 1024 || (nz->draws & (nz->draws - 1)) != 0)
        return iago_fail(IAGO_ERR_INVALID, (w + ": draws must be a power of two in [16, 1024]").c_str());
    if (!nz->counts)
        return iago_fail(IAGO_ERR_INVALID, (w + ": null counts buffer").c_str());
    return IAGO_OK;
}

// the urn across the 8 lanes of a game: the counts of this lane's 8 cells (8 l8 ..) after `draws` draws over the legal set
// lg, c[i] in 0 .. draws.  Every lane of the group takes part; lg with fewer than two cells: zeros, nothing drawn (the
// loop still runs while another game of the wave draws: `draws` is uniform)
__device__ __forceinline__ void noise_urn8(uint64_t lg, uint32_t l8, uint32_t key0, uint32_t key1, uint32_t id, uint32_t turn,
                                           uint32_t alpha_256, uint32_t draws, uint32_t (&c)[8])
{
    const bool urn = (lg & (lg - 1ull)) != 0ull;
    const uint32_t row = urn ? (uint32_t)(lg >> (8u * l8)) & 0xFFu : 0u;
    int wt[8]; // the weights alpha_256 + 256 c of this lane's legal cells, 0 off the legal set (< 2^20; their sum < 2^32)
#pragma unroll
    for (int i = 0; i < 8; i++)
        wt[i] = ((row >> i) & 1u) ? (int)alpha_256 : 0;
    if (__builtin_amdgcn_ballot_w64(urn) != 0ull) {
#pragma unroll 1
        for (uint32_t blk = 0u; blk < draws; blk += 4u) {
            uint32_t w[4] = {id, turn, blk >> 2, 0u};
            philox4x32_10(w, key0, key1 ^ NOISE_KEY);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint32_t a = (uint32_t)explore_draw8(wt, l8, w[q]); // (64 where the game draws nothing: no lane's cell)
#pragma unroll
                for (int i = 0; i < 8; i++)
                    wt[i] += (a == 8u * l8 + (uint32_t)i) ? 256 : 0;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 8; i++)
        c[i] = ((row >> i) & 1u) ? ((uint32_t)wt[i] - alpha_256) >> 8 : 0u;
}

// the mix of a root child's stored prior p (what init_node wrote: prior + the selection rule's prior_off) with its count c: p keep + term, keep =
// (256 - eps_256) / 256 and term = eps_256 c / (256 N) both exact in float32 (eps_256 c <= 2^18, N = 2^draws_log2), the
// product and the sum each rounded once, as numpy rounds them
__device__ __forceinline__ float noise_mix(float p, uint32_t c, uint32_t eps_256, uint32_t draws_log2)
{
#pragma clang fp contract(off)
    const float keep = (float)(256u - eps_256) * 0.00390625f;
    const float term = (float)(eps_256 * c) * __uint_as_float((127u - 8u - draws_log2) << 23);
    const float kept = p * keep;
    return kept + term;
}

// the mix on the EXISTING children of node `root` (a reused subtree: first child rfc >= 0, the children are the legal
// moves lg in ascending cell order, two or more): lane l8 rewrites the priors of its row's cells
__device__ __forceinline__ void noise_remix_children(const Tree &T, int64_t base, int rfc, uint64_t lg, uint32_t l8,
                                                     const uint32_t (&c)[8], uint32_t eps_256, uint32_t draws_log2)
{
    uint32_t row = (uint32_t)(lg >> (8u * l8)) & 0xFFu;
    int at = rfc + __popcll(lg & ((1ull << (8u * l8)) - 1ull));
#pragma unroll
    for (int i = 0; i < 8; i++) {
        if ((row >> i) & 1u) {
            T.nodes[base + at].p = noise_mix(T.nodes[base + at].p, c[i], eps_256, draws_log2);
            at++;
        }
    }
}

// ---- the Gumbel root search ("Gumbel root search"; the contract is iago_hip_serving.h's): the
// root's rule in integers, Q16.  The tables (gumbel_q16, ln_q16) and the schedule come from the host; nothing here calls log
// or exp
constexpr uint32_t GUMBEL_KEY = IAGO_GUMBEL_KEY; // ("GUMB")
constexpr int GUMBEL_LN2_Q16 = 45426;            // round(65536 ln 2)

// logit_q16 of a stored prior p > 0: (e - 127) round(65536 ln 2) + ln_q16[f >> 11] of its exponent and mantissa bits
__device__ __forceinline__ int gumbel_logit_q16(float p, const int32_t *__restrict__ ln_q16)
{
    const uint32_t b = __float_as_uint(p);
    return ((int)((b >> 23) & 0xFFu) - 127) * GUMBEL_LN2_Q16 + ln_q16[(b & 0x7FFFFFu) >> 11];
}

// q16 of a child with value q after n visits: 0 .. 65536 for q in [-1, 1] (q 32768 is exact in float32; ties to even)
__device__ __forceinline__ int gumbel_q16(float q, int n)
{
    return n > 0 ? (int)rintf(q * 32768.0f) + 32768 : 0;
}

// g + logit + sigma as a float64 (exact: below 2^53), sigma = ((c_visit + maxN) c_scale_256 q16) >> 8 in int64
__device__ __forceinline__ double gumbel_score(int g, int logit, int q16, int max_n, int c_visit, int c_scale_256)
{
    const int64_t sigma = ((int64_t)(c_visit + max_n) * (int64_t)c_scale_256 * (int64_t)q16) >> 8;
    return (double)((int64_t)g + (int64_t)logit + sigma);
}

// Diagnostic record of the parity tests (tests/test_mcts_production_gpu.py): the z every playout of game g backed up, in
// playout order -- what the oracle's rollout_fn replays (z_log [rows][n_games], z_log_n [n_games] rows written so far)
__device__ __forceinline__ void log_z(int8_t *z_log, int32_t *z_log_n, int rows, int64_t g, int64_t n_games, int8_t zg)
{
    const int k = z_log_n[g];
    z_log_n[g] = k + 1;
    if (k < rows)
        z_log[(int64_t)k * n_games + g] = zg;
}

} // namespace iago_mcts
