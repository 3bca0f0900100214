// search_kernel.hip -- a whole PV-MCTS search (n_sims playouts of every game: MCTS.get_move's loop,
// MCTS.py:139-147), or whole self-play games (the turn loop of game.py:117-142,253-255 around it), as
// ONE persistent launch in which every game runs on its own clock ("The persistent search":
// why, and the measurements behind its scheduling rules).  The chip is a pool of workgroups of two kinds:
//   * GAME workgroups (the first ceil(n_games / 32) of the grid: dispatched first, so always resident):
//     each owns 32 games, 8 lanes per game (a wave search: 32 slots, S.wave per tree).  game_workgroup is
//     a driver loop over phase functions: replies -> a playout's end -> the turn boundary of whole games
//     (the most visited move, the record, update_with_move, the stone and the books) -> descent (select,
//     expansion, pass chains; exactly descend_kernel's arithmetic) -> the control words -> rollout passes
//     of 16 boards (Philox stream = stream base + turn x n_sims + the game's own playout count) -> the
//     wave's backups -> the iteration's end (pacing, abort) -> a stream's claim of the next games.  A leaf
//     without a stored value (that the shared position table does not hold) or a node that expands
//     (n_visits >= n_thr, MCTS.py:109) sends a request to a ring and the game waits for the reply while
//     its rollout runs and the workgroup's other games go on.
//   * NET workgroups (the rest of the grid): each takes a ticket of a ring that has an entry waiting
//     (its home ring first: one ring per net), walks the board through the Value net (trunk_item<true, 1>,
//     or <true, 2> for two entries together) or the SLPolicy net (policy_item) -- the kernels' own device
//     functions: bit-identical numbers -- and publishes the result in the game's mailbox (and the table).
// A game's sequence of playouts -- leaves, values, priors, rollouts, backups, expansions, moves -- is
// exactly the reference's; only the interleaving between games changes: trees, moves and results are
// bit-identical to the per-playout engine's (tests/test_search_persistent_gpu.py; the comparisons with
// the oracle's MCTS.py restatement in tests/test_mcts_production_gpu.py run on this kernel).
//
// Inter-workgroup traffic (cdna_hip_programming.md, guideline 16, form R2): every shared word is an
// 8-byte {tag, 32-bit value} granule written by ONE agent-scope atomic store and polled by agent-scope
// atomic loads -- the data is the flag, no fence, no cache invalidation that would cost the net
// workgroups their L2-resident weights.  Ring entry t (ticket t, tag t + 1): 6 granules (kind | game,
// reply tag, the position's four words); replies: one granule (value) or 64 (priors) tagged with the
// request's reply tag (search_request.hpp states both layouts, for this file and the walks).  The tree, the cursors and the paths of a game are touched by its own workgroup
// only.  Every wait is a bounded poll: the launch ends by itself when a clock limit passes (abort word).
#include "mcts_dev.hpp"
#include "conv_trunk_body.hpp" // (brings rollout_row_body.hpp)
#include "conv_policy_body.hpp"
#include "sample_dev.hpp"
#include "search_request.hpp"
#include "../../include/iago_hip_serving.h"

#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <string>
#include <vector>

namespace {
using namespace iago;
using namespace iago_mcts;

typedef unsigned long long u64;
#define RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

constexpr uint32_t QCAP = IAGO_SEARCH_QUEUE_ENTRIES; // entries of a request ring (a game has at most ONE request outstanding:
                                                     // >= the 4096 games a launch can hold)
constexpr int CTL_FINISHED = 2, CTL_ABORT = 3;
// two request rings, one per kind of net work: head (tickets handed out) / tail (entries reserved) of ring q
__host__ __device__ constexpr int ctl_head(uint32_t q) { return 8 + 2 * (int)q; }
__host__ __device__ constexpr int ctl_tail(uint32_t q) { return 9 + 2 * (int)q; }
enum { ST_READY = 0, ST_WAIT_PRIOR, ST_PRIOR_READY, ST_ROLL, ST_ROLL_FRESH, ST_WAIT_VALUE, ST_HAVE_VALUE, ST_DONE, ST_TURN, ST_MOVE,
       ST_WAIT_DRAW, ST_DRAW,   // (a match: the policy side waits for its move's distribution, then draws)
       ST_IDLE };               // (a wave search: a slot without a playout in its tree's current wave)
constexpr int CTL_NO_CHILDREN = 4; // a searched root had no children (n_sims below n_thr)
constexpr uint32_t MATCH_KEY = 0x4D415443u; // ("MATC") a match's policy draws: the rollout key's high word XOR this
constexpr int CTL_BAD_DRAW = 13;   // a match: a policy draw found no probability mass on the legal moves (NaN / zero)
// pacing (below): sum over the games in play of their progress (turn x n_sims + playouts of the turn), games in play
constexpr int CTL_PROGRESS = 5, CTL_PLAYING = 6;
constexpr int CTL_NET_WGS = 7;            // net workgroups of this launch (written by the launch: the grid follows the device)
constexpr int CTL_IDLE = 14;              // net workgroups that found nothing to do at their last look (they poll)
constexpr int CTL_NEXT_GAME = 12;         // a stream: game ids claimed beyond the first fill (the next one: n_games + this)
// a request's words, a ring's granules and a mailbox's: search_request.hpp (the walks read a request, too)
namespace rq = iago_request;
using rq::KIND_POLICY;
using rq::KIND_VALUE;
using rq::NOBODY;
// games of a GAME workgroup: 8 lanes per game in the descent and the backup (16 games = two waves, 32 = all four),
// rollouts in passes of 16 boards (the 16-lanes-per-board body)
constexpr int GAMES_PER_WG = IAGO_SEARCH_GAMES_PER_WORKGROUP; // at most (the launch's own number: SearchParams::games_per_wg)

// dynamic LDS of the kernel: the walks' images (the larger of a value pair's and a policy board's, with their heads), then
// block1's weights of both nets
constexpr int SEARCH_IMG_V = iago_trunk::lds_alloc(2) + iago_trunk::head_lds(2);
constexpr int SEARCH_IMG_P = iago_policy::BS + 1024 + iago_policy::HEAD_FLOATS * 4;
constexpr int SEARCH_IMG_TOP = SEARCH_IMG_V > SEARCH_IMG_P ? SEARCH_IMG_V : SEARCH_IMG_P;

struct SearchParams {
    Tree T;
    const uint64_t *root_own, *root_opp;
    const uint8_t *active;
    float c_puct, lmbda;
    int32_t n_thr, n_sims, n_game_wgs, games_per_wg;
    int32_t *cur_node;
    uint64_t *cur_own, *cur_opp;
    int32_t *path;
    int32_t path_stride;
    int32_t *done;
    uint8_t *roll;
    int8_t *z;
    float *leaf_value;
    int8_t *z_log;
    int32_t *z_log_n;
    int32_t z_log_rows;
    u64 *q_slots;
    uint32_t *ctl;
    u64 *rep_v, *rep_p;
    int64_t *totals; // [0] value evaluations, [1] policy evaluations, [2] game-workgroup iterations, [3] pair walks,
                     // [4] / [5] net workgroups' waiting / walking time (100 MHz ticks), [6] idle game iterations, [7] game time
    int32_t *stats;
    uint64_t *wg_own, *wg_opp;
    long long clock_limit; // wall_clock64 ticks (100 MHz) after which the launch gives up
    // whole self-play games in the launch (iago_selfplay_persistent): max_turns > 0.  A game then walks through
    // its turns on its own: legal moves of the mover, a search of n_sims playouts (or a pass), the most visited
    // move (MCTS.get_move, MCTS.py:147), MCTS.update_with_move (MCTS.py:149-154), the move on the board and the
    // turn bookkeeping of game.py:117-142,253-255 -- what SelfPlayEngine.play drives per turn for all games
    int32_t max_turns;
    uint64_t *game_own, *game_opp;   // [n_games] in: the start positions (own = colour 1, the first mover); out: final
    int32_t *n_turns;                // [n_games] out: turns the game took (even, or max_turns)
    uint64_t *rec_own, *rec_opp;     // optional [max_turns][n_games]: the position before every turn (own = mover)
    uint8_t *rec_valid;              // [max_turns][n_games]: the mover had a move and searched
    int8_t *rec_move;                // [max_turns][n_games]: the move played, -1 = pass / no turn
    int32_t *rec_pi;                 // [max_turns][n_games][64]: the root's visit counts by action
    // a self-play STREAM (stream != 0): games_total games in the launch, at most n_games (the slots) of them in play; a game
    // workgroup whose games are all over claims the next game ids (CTL_NEXT_GAME), one per slot, resets the slots' trees and
    // plays those games from their first turn.
    // game_own / game_opp / n_turns are then [games_total] and the records [max_turns][games_total], indexed by the GAME;
    // the rollouts draw with the game's id.  Not a stream: games_total = n_games, game = slot
    int32_t games_total, stream;
    // optional position table shared by all games and launches: value_func(state) is a pure function of the position, and
    // games that start from one position keep meeting each other's positions (9.5 % of the value requests of 1024 games
    // x 100 playouts repeat a position asked for before: LABNOTES.md).  Direct-mapped, 32-byte entries {seq, own, opp,
    // value bits} under a per-entry sequence lock, every word an agent-scope atomic
    u64 *vtable;           // nullptr = no table
    uint32_t vtable_mask;  // slots - 1 (slots a power of two; 0: ONE slot, every position's -- never the sign of "no table")
    int64_t *trace;        // optional diagnostic [trace_rows][4]: game workgroup 0 samples (ticks, tail, head, finished) per iteration
    int32_t trace_rows;
    int32_t policy_xcds;   // XCDs (of 8) whose workgroups serve the POLICY ring first
    int32_t pair_backlog;  // entries that must be waiting (beyond the tickets handed out) for a net workgroup to take two
    // pacing: a game that is more than `pace_margin` playouts ahead of the mean progress of the games in play starts no
    // new playout while more than `pace_backlog` requests wait in the rings (< 0: no pacing).  Why: the batch ends with
    // its slowest game, and a game's speed in the net-bound middle of a batch is set by how many requests it makes (end
    // time against requests sent: correlation 0.84-0.90, ends spread over +-20 % at 400 playouts per move; LABNOTES.md);
    // what the leaders do not ask for, the laggards get.  Timing only: a game's own sequence of playouts is untouched
    int32_t pace_margin, pace_backlog;
    // values ahead of their first visit, on idle hands only: when a game asks for the priors of a node that expands while
    // at least `ahead_idle` net workgroups poll and nothing waits in the rings, the node's children (each of them a leaf
    // without a value at ITS first visit: the first in this very playout, the others a few playouts from now) are walked
    // through the value net beside the policy walk and put into the position table (< 0: off; needs the table)
    int32_t ahead_idle;
    int32_t roll_defer; // rollouts: games a full pass of 16 may leave over for the next iteration (0: every game at once)
    int32_t path_lds_cap; // bytes of the launch's dynamic LDS a game workgroup may keep its games' recorded paths in
    // the wave search (iago_mcts_search_wave, search_wave_kernel): `wave` slots per tree, n_slots = trees x wave
    int32_t wave;
    float vloss;
    int64_t n_slots;
    int64_t *wave_timing;
    // the hand-over of iago_mcts_search_park (the PARK instantiations alone read these): a self-play game whose turn would
    // be searched at a position of at most park_empties empties writes its books here, by game id, and is done
    int32_t park_empties;
    uint8_t *parked;
    int32_t *park_stones;
    uint8_t *park_pass;
    // exploring self-play (iago_mcts_search_explore; 0: off): the move of a searched turn below explore_turns is drawn in
    // proportion to the root's visit counts (mcts_dev.hpp, explore_draw8) instead of taken as the most visited one
    int32_t explore_turns;
    // playout-cap randomisation (iago_mcts_search_cap; cap_fast 0: off): a searched turn whose Philox word says FAST
    // (mcts_dev.hpp, cap_word: top byte >= cap_full_256) ends its search after cap_fast playouts and records valid 4
    int32_t cap_fast, cap_full_256;
    // the descent jumps over a pass chain it remembers from the game's last playout (descend; IAGO_SEARCH_CHAIN_SKIP):
    // timing only.  totals[16] then counts the levels jumped over
    int32_t chain_skip;
    // root noise (iago_mcts_search_noise; the NOISE instantiations alone read these): eps_256, log2 of the urn's draws and
    // the counts rows [n_games][64] that iago_mcts_root_noise wrote before the launch, read where a root expands
    uint16_t *noise_counts;
    int32_t noise_eps, noise_lg;
    // forced playouts (iago_mcts_search_forced; the NOISE instantiations alone read it): k_256, 0 = none forced
    int32_t forced_k_256;
    // the backup rule (backup_game; IAGO_SEARCH_NEGAMAX): 0 = the reference's, the leaf's value at every level of the path;
    // 1 = negamax, its sign turned from level to level (mcts_dev.hpp, backup_value)
    int32_t negamax;
    // the selection rule (mcts_dev.hpp, "the selection rule"; IAGO_SEARCH_PUCT_AZ): what a new child's stored prior adds to
    // the policy's output, and what the exploration term's denominator adds to the visits.  0.1f and 0.01: the
    // reference's; 0.0f and 1.0: AlphaZero's.  Uniform over the launch: scalar operands, no branch, no instantiation.
    // (The struct's last fields: prior_off fills the padding after negamax, visit_off adds 8 bytes, by which the kernel
    // parameters after a SearchParams move)
    float prior_off;
    double visit_off;
    // the Gumbel root search (iago_mcts_search_gumbel; the ROOT_GUMBEL instantiations alone read these): the draws by cell
    // [n_games][64] that iago_mcts_gumbel_draw wrote before the launch, the host's ln table and schedule [m + 1][n_sims],
    // the moves considered and the two constants of sigma.  (After visit_off: the plain kernels' fields stay where they were)
    const int32_t *gumbel_g, *gumbel_ln;
    const int16_t *gumbel_sched;
    int32_t gumbel_m, gumbel_c_visit, gumbel_c_scale;
};

// The rule at the root of a search (the path's first node), by instantiation: none, root noise with forced playouts
// (iago_mcts_search_noise / _forced), the Gumbel rule (iago_mcts_search_gumbel).  The plain kernels compile none of it.
constexpr int ROOT_PLAIN = 0, ROOT_NOISE = 1, ROOT_GUMBEL = 2;

__device__ __forceinline__ u64 ld(const u64 *p) { return __hip_atomic_load(p, RLX_AGENT); }
__device__ __forceinline__ void st(u64 *p, u64 x) { __hip_atomic_store(p, x, RLX_AGENT); }

// ---- the request rings (one per kind of net work).  Game lanes write them (send_request), wave 0 of a net workgroup
// reads them (ring_backlog, ring_take, ring_fetch).
__device__ __forceinline__ u64 *ring_entry(const SearchParams &S, uint32_t q, uint32_t t)
{
    return S.q_slots + ((u64)q * QCAP + t % QCAP) * (u64)rq::SLOT_STRIDE;
}

// one request: the granules of entry `t` (one lane)
__device__ __forceinline__ void send_request(const SearchParams &S, uint32_t kind, int64_t g, uint32_t reply_tag,
                                             uint64_t own, uint64_t opp)
{
    const uint32_t t = __hip_atomic_fetch_add(&S.ctl[ctl_tail(kind)], 1u, RLX_AGENT);
    // (ring_entry written out: through the helper the game kernels are the same instructions in another allocation,
    // 3 to 5 more spilled SGPRs: LABNOTES.md, "The net workgroup in named phases")
    u64 *e = S.q_slots + ((u64)kind * QCAP + t % QCAP) * (u64)rq::SLOT_STRIDE;
    st(e + rq::W_TAG, rq::entry_word(t, reply_tag));
    st(e + rq::W_OWN_LO, rq::entry_word(t, (uint32_t)own));
    st(e + rq::W_OWN_HI, rq::entry_word(t, (uint32_t)(own >> 32)));
    st(e + rq::W_OPP_LO, rq::entry_word(t, (uint32_t)opp));
    st(e + rq::W_OPP_HI, rq::entry_word(t, (uint32_t)(opp >> 32)));
    st(e + rq::W_WHO, rq::entry_word(t, rq::who_word(kind, (uint32_t)g)));
    atomicAdd((unsigned long long *)&S.totals[(uint32_t)g == NOBODY ? 11 : kind], 1ull);
}

// (wave 0, uniform; lane 0 looks) the search is over -- every game workgroup has finished: no request can come any
// more --, aborted, or past its clock
__device__ __forceinline__ bool search_over(const SearchParams &S, const long long t0)
{
    bool out = false;
    if (threadIdx.x == 0)
        out = __hip_atomic_load(&S.ctl[CTL_FINISHED], RLX_AGENT) >= (uint32_t)S.n_game_wgs ||
              __hip_atomic_load(&S.ctl[CTL_ABORT], RLX_AGENT) != 0u || wall_clock64() - t0 > S.clock_limit;
    return __builtin_amdgcn_ballot_w64(out) != 0ull;
}

// Tickets are handed out by fetch-and-add whenever the ring shows an entry waiting: several workgroups that saw the
// same entry all take one, and the later ones wait in ring_fetch for the ring's next entries.  (Measured and dropped,
// round 5: head moved by compare-and-swap bounded by the tail, so that nobody is committed to an entry that does not
// exist -- a retry loop took the 1024-game batch from 0.39 to 3.6 s, one attempt per look to 1.76 s: the losers keep
// polling and retrying on ONE word from all XCDs, same-address atomics serialise, and every claim queues behind them.)
// (wave 0, uniform; lane 0 looks) entries of ring q beyond the tickets handed out
__device__ __forceinline__ int ring_backlog(const SearchParams &S, uint32_t q)
{
    int d = 0;
    if (threadIdx.x == 0)
        d = (int32_t)(__hip_atomic_load(&S.ctl[ctl_tail(q)], RLX_AGENT) - __hip_atomic_load(&S.ctl[ctl_head(q)], RLX_AGENT));
    return __builtin_amdgcn_readfirstlane(d);
}
// (wave 0, uniform) the next ticket of ring q
__device__ __forceinline__ uint32_t ring_take(const SearchParams &S, uint32_t q)
{
    uint32_t t = 0;
    if (threadIdx.x == 0)
        t = __hip_atomic_fetch_add(&S.ctl[ctl_head(q)], 1u, RLX_AGENT);
    return __builtin_amdgcn_readfirstlane(t);
}
// wave 0: wait for entry t of ring q (at most max_spins polls; 0 = until it comes or the search is over)
// -> dst[0 .. WORDS) (LDS); returns 0 = entry read, 1 = not there yet, 2 = the search is over / given up
__device__ __forceinline__ int ring_fetch(const SearchParams &S, uint32_t q, uint32_t t, uint32_t max_spins, uint32_t *dst,
                                          const long long t0)
{
    const int tid = threadIdx.x;
    const u64 *e = ring_entry(S, q, t);
    u64 x = 0;
    int status = 0;
    for (uint32_t spins = 0;; spins++) {
        x = (tid < rq::WORDS) ? ld(e + tid) : 0ull;
        const bool ok = tid >= rq::WORDS || rq::entry_is(x, t);
        if (__builtin_amdgcn_ballot_w64(ok) == ~0ull)
            break;
        if (max_spins && spins + 1u >= max_spins) {
            status = 1;
            break;
        }
        if ((spins & 15u) == 15u && search_over(S, t0)) {
            status = 2;
            break;
        }
        __builtin_amdgcn_s_sleep(8);
    }
    if (status == 0 && tid < rq::WORDS)
        dst[tid] = (uint32_t)x;
    return status;
}

// the replies (one lane per granule): a value into the mailbox of the game that waits for it (nobody: into none);
// word i of a distribution
__device__ __forceinline__ void reply_value(const SearchParams &S, const uint32_t *r, uint32_t bits)
{
    if (rq::game(r) != NOBODY)
        st(&S.rep_v[(int64_t)rq::game(r)], rq::reply_word(rq::tag(r), bits));
}
__device__ __forceinline__ void reply_prior(const SearchParams &S, const uint32_t *r, int i, uint32_t bits)
{
    st(&S.rep_p[(int64_t)rq::game(r) * 64 + i], rq::reply_word(rq::tag(r), bits));
}

__device__ __forceinline__ uint32_t vtable_slot(const SearchParams &S, uint64_t own, uint64_t opp)
{
    uint64_t h = own * 0x9E3779B97F4A7C15ull ^ (opp + 0xD1B54A32D192ED03ull) * 0xBF58476D1CE4E5B9ull;
    h ^= h >> 29;
    h *= 0x94D049BB133111EBull;
    h ^= h >> 32;
    return (uint32_t)h & S.vtable_mask;
}

// value of the position if the table holds it (one lane); the five loads are in flight together, the entry counts only
// if its sequence word is even and did not move
__device__ __forceinline__ bool vtable_get(const SearchParams &S, uint64_t own, uint64_t opp, uint32_t &bits, uint32_t &writer)
{
    const u64 *e = S.vtable + (u64)vtable_slot(S, own, opp) * 4u;
    const u64 s1 = ld(e), o = ld(e + 1), p = ld(e + 2), v = ld(e + 3);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); // (compiler order only: the words are agent-scope atomics)
    const u64 s2 = ld(e);
    bits = (uint32_t)v;
    writer = (uint32_t)(s1 >> 32);
    return s1 != 0ull && (s1 & 1ull) == 0ull && s1 == s2 && o == own && p == opp && (v >> 32) == (s1 & 0xFFFFFFFFull);
}

// (one lane) the value the net has just computed for the position, in two steps.  vtable_put_begin takes the slot with
// ONE atomic (fetch-or of the sequence word's low bit: odd = being written; a slot somebody else is writing is left
// alone) and stores the position and the value; vtable_put_end -- called by the same lane before its next request, a
// walk later -- publishes the new even sequence word once those stores have landed.  (As one routine -- load, compare-and-
// swap, stores, wait, store -- it was three dependent round trips to L2 behind every value walk: LABNOTES.md, round 5.)
// Sequence word: low half = the sequence number (odd while the entry is being written, never 0 once used), high half =
// the game whose request put the value there (diagnostic: hits by the same game / by another game, totals[12])
__device__ __forceinline__ u64 *vtable_put_begin(const SearchParams &S, uint64_t own, uint64_t opp, uint32_t bits, uint32_t writer,
                                                 u64 &publish)
{
    u64 *e = S.vtable + (u64)vtable_slot(S, own, opp) * 4u;
    const u64 s = __hip_atomic_fetch_or(e, 1ull, RLX_AGENT);
    if (s & 1ull)
        return nullptr;
    uint32_t seq = (uint32_t)s + 2u;
    seq = seq ? seq : 2u;
    st(e + 1, own);
    st(e + 2, opp);
    st(e + 3, ((u64)seq << 32) | bits);   // (the value word carries the sequence number it belongs to)
    publish = ((u64)writer << 32) | seq;
    return e;
}
__device__ __forceinline__ void vtable_put_end(u64 *e, u64 publish)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    st(e, publish);
}

template <int CTRL>
__device__ __forceinline__ void most_visited_step(int &n, int &a)
{
    const int on = (int)dpp_u32<CTRL>((uint32_t)n), oa = (int)dpp_u32<CTRL>((uint32_t)a);
    const bool take = on > n || (on == n && oa < a);
    n = take ? on : n;
    a = take ? oa : a;
}

__device__ __forceinline__ bool group8_all(bool x)
{
    return group8_add(x ? 0u : 1u) == 0u;
}

// A match's policy move (game.py:100-104): sample_wave's draw from the 64 replies of the game's mailbox -- p = prob x valid /
// sum, float64 sums in cell order, the first cell whose cdf / cdf[-1] exceeds u -- run whole by every lane of the game (8
// lanes, no LDS row to share): bit-identical to sample_moves.  64: no mass on the legal moves (NaN / inf / zero)
__device__ __forceinline__ int policy_draw(const u64 *rep, uint64_t lg, double u)
{
    double s = 0.0; // np.sum(prob * valid)
#pragma unroll 1
    for (int j = 0; j < 64; j++)
        s += ((lg >> j) & 1ull) ? (double)__uint_as_float(rq::reply_bits(ld(rep + j))) : 0.0;
    double last = 0.0; // cumsum(p / s)[-1]
#pragma unroll 1
    for (int j = 0; j < 64; j++)
        last += (((lg >> j) & 1ull) ? (double)__uint_as_float(rq::reply_bits(ld(rep + j))) : 0.0) / s;
    if (!(s > 0.0) || !(s <= 1.7976931348623157e308) || !(last > 0.0))
        return 64;
    double acc = 0.0;
    int n = 0; // searchsorted(cdf, u, side='right')
#pragma unroll 1
    for (int j = 0; j < 64; j++) {
        acc += (((lg >> j) & 1ull) ? (double)__uint_as_float(rq::reply_bits(ld(rep + j))) : 0.0) / s;
        n += acc / last <= u ? 1 : 0;
    }
    return n;
}

// entry d of a game's recorded path: in the workgroup's LDS from word path_at (>= 0; an LDS access, not a flat one), else in
// the caller's array
__device__ __forceinline__ int path_entry(int path_at, const int32_t *gpath, int d)
{
    return path_at >= 0 ? ((const int32_t *)iago_trunk::trunk_lds)[path_at + d] : gpath[d];
}

// Node.update_recursive over the recorded path + the leaf mix, as mix_backup_path_kernel does them: 8 lanes per game.
// g: the slot (its path, its leaf value), gt: its tree (the same
// unless a wave search, which also takes the playout's in-flight visit off every node of the path)
template <bool WAVE>
__device__ __forceinline__ void backup_game(const SearchParams &S, int64_t g, uint32_t r, int leaf, bool fresh, float vg,
                                            int path_n, const int8_t zl, const int negamax, const int path_at,
                                            const int64_t gt)
{
    const int64_t base = gt * (int64_t)S.T.capacity;
    const float lmbda = S.lmbda;
    if (fresh && lmbda < 1.0f && r == 0u)
        S.T.nodes[base + leaf].v = vg; // value_func(leaf), now stored (the value cache)
    const int8_t zg = lmbda > 0.0f ? zl : (int8_t)0; // (the rollout's result, from the workgroup's LDS)
    const float lv = leaf_mix(lmbda, vg, zg);
    if (r == 0u) {
        S.leaf_value[g] = lv;
        if (S.z_log && lmbda > 0.0f)
            log_z(S.z_log, S.z_log_n, S.z_log_rows, gt, S.T.n_games, zg);
    }
    const int len = path_n < S.path_stride ? path_n : S.path_stride;
    const int32_t *const gpath = S.path + g * (int64_t)S.path_stride;
    // (the backup rule: a lane's indices d = r, r + 8, .. are of one parity, so one value per lane; the parity is that of
    // the path's true length path_n, not of the `len` the buffer holds.  The reference's rule: lv itself.  `negamax`:
    // S.negamax, from the workgroup's LDS)
    const float lvd = backup_value(negamax, lv, path_n, (int)r);
    for (int d = (int)r; d < len; d += 8) {
        const int node = path_entry(path_at, gpath, d);
        visit(S.T, base + node, lvd);
        if constexpr (WAVE)
            S.T.nodes[base + node].reserved1 -= 1; // vv: this playout is no longer in flight
    }
}

// a barrier that also orders the workgroup's global stores before it against its loads after it (workgroup-scope
// release / acquire): how the slots of a wave search hand a tree to each other (cdna_hip_programming.md, guideline 16)
__device__ __forceinline__ bool wg_handoff_or(bool x)
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    const bool any = __syncthreads_or(x) != 0;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    return any;
}

// The games of a GAME workgroup (8 lanes per game: 32 games = the four waves).
// WAVE (iago_mcts_search_wave): the 8-lane groups are SLOTS, S.wave consecutive ones per tree (32 per workgroup: a tree
// never straddles two), and a slot plays one playout of its tree's current wave.  Its descent waits for the slot before
// it (the tree's `wv_next`, handed over with wg_handoff_or), its leaf is evaluated as in the plain search, and the
// wave's backups run in slot order once every leaf of the wave has its value.
// game_workgroup is a driver loop over the phases below; every phase function is called by all threads of the workgroup
// or, where it says so, by the lanes of the games (`mine`: whole waves).

// a thread of a game workgroup: its game (a wave search: its slot and tree), its place in the group of 8, its path
struct Slot {
    int tid, gl;          // the thread, its game's number within the workgroup
    int wg;               // the workgroup's number among its search's game workgroups (blockIdx.x unless an arena launch)
    uint32_t r;           // lane within the game's 8
    Lane8 L;
    bool mine, exists;    // a lane of one of the workgroup's games (a wave search: every thread); that game exists
    int64_t g, gt, base;  // the slot, its tree (the same unless a wave search), the tree's first node
    int64_t n_slots;
    int W, s_in, tl;      // a wave search: slots per tree, slot within the tree, tree within the workgroup
    int path_at;          // word of the dynamic LDS where this game's path starts (-1: in the caller's array)
    int32_t *gpath;
    bool whole, need_v, need_z;
    int search_end;       // where a game goes when its search's last playout is backed up
};

// a game and its books: its state, the reply tag of its last request (never 0 once used), the playouts of its current
// search; with whole games its turn, its books (game.py:32,117-142) and its own position (own = side to move)
struct Game {
    int state;
    uint32_t epoch;
    int n_done, turn, stones;
    bool pass_flg, g_over;
    uint64_t g_own, g_opp;
};

// the descent's cursor (kept across iterations while the game waits for priors): the node, its first child, children,
// visits, in-flight visits (a wave search) and stored value bits, the position there, the path's length; the leaf reached,
// whether the node may still expand, whether the leaf had no stored value, and the value that came back for it
struct Cursor {
    int node, fc, k, nv, nvv;
    uint32_t vbits;
    uint64_t own, opp;
    int path_n, leaf;
    bool may_expand, leaf_fresh;
    float v_reply;
};

// the static LDS of a game workgroup, declared once
struct GameLds {
    // positions, Philox stream offsets and results between the descent / backup and the rollout passes (RowHandoff)
    uint64_t h_own[GAMES_PER_WG], h_opp[GAMES_PER_WG];
    int32_t h_stream[GAMES_PER_WG];
    int32_t h_game[GAMES_PER_WG]; // the game each slot plays (the slot itself unless a stream), read at its end
    // the playouts of each slot's current search (S.n_sims; a fast turn of the playout cap: S.cap_fast) and whether the
    // turn is a fast one -- in LDS like the two above: the kernel has no register left for a per-game word
    int32_t h_budget[GAMES_PER_WG];
    uint8_t h_fast[GAMES_PER_WG];
    // (diagnostic counters of the workgroup, kept by thread 0 in LDS: as per-thread 64-bit registers they were 12 VGPRs
    // live across the whole loop -- what the game launch of the role split spilled to scratch memory)
    uint32_t wg_count[7]; // [0] iterations, [1] idle iterations, [2..5] iterations with 0 / 1..16 / 17..20 / more games rolled out,
                          // [6] levels of remembered pass chains the descents jumped over
    // the pass chain at the end of each game's last recorded path (descend): ch_from = the first path index from which
    // every step down to the path's last entry (index ch_len - 1) went from a node with ONE child to that child, a pass
    // (-1: nothing remembered); ch_run: the same index for the path being recorded
    int32_t ch_from[GAMES_PER_WG], ch_len[GAMES_PER_WG], ch_run[GAMES_PER_WG];
    int32_t roll_list[GAMES_PER_WG]; // games whose leaf is rolled out in this iteration, packed
    uint32_t roll_wave[BLOCK / 64], roll_wave_old[BLOCK / 64];
    // pacing: the workgroup's changes of CTL_PROGRESS / CTL_PLAYING in an iteration, which go out as one atomic each;
    // pace[2]: the progress above which a game holds; pace[3]: the iteration's budget of requests nobody waits for
    int32_t pace[4];
    uint32_t claimed; // a stream: the first game id of the block the workgroup claimed
    // S.negamax, read by the backups from here: as a kernel argument it is one more scalar kept (and spilled) across the
    // whole loop
    int32_t negamax;
    int8_t h_z[GAMES_PER_WG];
};
// a wave search adds, per tree of the workgroup, the slots of its current wave that have descended (the next one to go),
// the wave's playouts, whether a slot of the wave still waits for its leaf's evaluation
template <bool WAVE> struct GameShared : GameLds {};
template <> struct GameShared<true> : GameLds {
    int32_t wv_next[GAMES_PER_WG], wv_size[GAMES_PER_WG], wv_block[GAMES_PER_WG];
    long long wv_time[4]; // (diagnostic, thread 0: descents, rollouts, backups, waits; S.wave_timing)
};

template <bool WAVE>
__device__ __forceinline__ Slot make_slot(const SearchParams &S, const int wg)
{
    Slot I;
    I.wg = wg;
    I.tid = threadIdx.x;
    I.gl = I.tid >> 3;
    I.L = make_lane8(threadIdx.x);
    I.r = I.L.l8;
    I.mine = I.tid < 8 * S.games_per_wg; // (WAVE: 32 slots, every thread)
    I.g = (int64_t)wg * S.games_per_wg + I.gl;
    I.W = WAVE ? S.wave : 1;
    I.n_slots = WAVE ? S.n_slots : S.T.n_games;
    I.exists = I.mine && I.g < I.n_slots;
    I.gt = WAVE ? I.g / I.W : I.g;
    I.s_in = WAVE ? (int)(I.g % I.W) : 0;
    I.tl = WAVE ? I.gl / I.W : 0;
    I.base = I.exists ? I.gt * (int64_t)S.T.capacity : 0;
    I.need_v = S.lmbda < 1.0f;
    I.need_z = S.lmbda > 0.0f;
    // the descent's recorded path (Node.update_recursive's ancestors): in the workgroup's dynamic LDS -- a game workgroup
    // walks no net while it has games -- when 32 paths fit there, else in the caller's array.  (From global memory the
    // backup was two dependent round trips to L2: the path entry, then the node.)
    const bool path_lds = (size_t)S.games_per_wg * (size_t)S.path_stride * 4u <= (size_t)S.path_lds_cap;
    I.path_at = path_lds ? I.gl * S.path_stride : -1;
    I.gpath = S.path + (I.exists ? I.g : 0) * (int64_t)S.path_stride;
    I.whole = S.max_turns > 0;
    I.search_end = I.whole ? ST_MOVE : ST_DONE;
    return I;
}

// a game's start (game.py:32): its position (own = colour 1, the first mover), its books, no playouts yet
__device__ __forceinline__ void start_game(Game &G, uint64_t own, uint64_t opp)
{
    G.g_own = own;
    G.g_opp = opp;
    G.turn = 0;
    G.stones = 4;
    G.pass_flg = false;
    G.g_over = false;
    G.n_done = 0;
}

// the cursor at `node`: an = action | n_children << 8, vv its in-flight visits (a wave search)
template <bool WAVE>
__device__ __forceinline__ void cursor_to(Cursor &C, int node, uint32_t fc, uint32_t nv, uint32_t an, uint32_t vv, uint32_t vbits)
{
    C.node = node;
    C.fc = (int)fc;
    C.k = (int)((an >> 8) & 0xFFu);
    C.nv = (int)nv;
    if (WAVE)
        C.nvv = (int)vv;
    C.vbits = vbits;
}

// the end of a playout of the plain search: the backup, the count, the rollouts' Philox stream of the next one
__device__ __forceinline__ void finish_playout(const SearchParams &S, const Slot &I, const GameLds &sh, Game &G,
                                               const Cursor &C, bool fresh, float v)
{
    backup_game<false>(S, I.g, I.r, C.leaf, fresh, v, C.path_n, sh.h_z[I.gl], sh.negamax, I.path_at, I.g);
    G.n_done++;
    if (S.trace && I.r == 0u)
        atomicAdd((unsigned long long *)&S.totals[9], 1ull); // (diagnostic: playouts over time)
    if (I.r == 0u)
        S.done[I.g] = G.turn * S.n_sims + G.n_done;
    G.state = G.n_done >= sh.h_budget[I.gl] ? I.search_end : ST_READY;
}

// ---- 1. replies (the games' lanes): the priors, a match's policy distribution, or the value the game waits for.  (The 8
// lanes of a game load the same word in the same instruction, or agree through group8_all: one state per game)
__device__ __forceinline__ void take_replies(const SearchParams &S, const iago_row::HwParams &R, const Slot &I,
                                             const GameLds &sh, Game &G, Cursor &C)
{
    if (G.state == ST_WAIT_PRIOR || G.state == ST_WAIT_DRAW) {
        bool ok = true;
#pragma unroll
        for (int i = 0; i < 8; i++)
            ok = ok && rq::reply_tag(ld(&S.rep_p[I.g * 64 + (int)I.r * 8 + i])) == G.epoch;
        if (group8_all(ok)) {
            if (G.state == ST_WAIT_DRAW) {
                // np.random.choice(64, p=prob*valid/np.sum(prob*valid)) (game.py:102-104) with the uniform of
                // (seed ^ MATCH_KEY << 32, game id, turn, stream 0): ops.sample_moves' draw.  (The move waits in
                // `leaf`, which no search of this game reads before the move is played)
                const uint64_t lg = group8_legal(to_lane(G.g_own, I.L), to_lane(G.g_opp, I.L), I.L);
                const double u = sample_uniform(R.key0, R.key1 ^ MATCH_KEY, R.id_base + (uint32_t)sh.h_game[I.gl],
                                                (uint32_t)G.turn, 0u);
                C.leaf = policy_draw(S.rep_p + I.g * 64, lg, u);
                if (C.leaf == 64) { // (numpy raises: the engine does, from this flag; the game goes on meanwhile)
                    if (I.r == 0u)
                        __hip_atomic_store(&S.ctl[CTL_BAD_DRAW], 1u, RLX_AGENT);
                    C.leaf = (int)__builtin_ctzll(lg);
                }
            }
            G.state = G.state == ST_WAIT_PRIOR ? ST_PRIOR_READY : ST_DRAW;
        }
    } else if (G.state == ST_WAIT_VALUE) {
        const u64 x = ld(&S.rep_v[I.g]);
        if (rq::reply_tag(x) == G.epoch) {
            C.v_reply = __uint_as_float(rq::reply_bits(x));
            G.state = ST_HAVE_VALUE;
        }
    }
}

// MCTS.get_move's most visited child of the root (MCTS.py:147) -- the root's children are the mover's legal moves in
// ascending order (Node.expand) --: -2 if it has none.  row_n: the visit counts of this lane's 8 actions
__device__ __forceinline__ int most_visited(const Tree &T, const Slot &I, uint64_t lg, int rfc, bool at_move, int (&row_n)[8])
{
    int best_n = -1, best_a = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int a = (int)(8u * I.r) + i;
        int n = 0;
        if (at_move && rfc >= 0 && ((lg >> a) & 1ull)) {
            n = T.nodes[I.base + rfc + __popcll(lg & ((1ull << a) - 1ull))].n_visits;
            if (n > best_n) { // the first maximum wins (MCTS.py:147)
                best_n = n;
                best_a = a;
            }
        }
        row_n[i] = n;
    }
    // argmax over the 8 lanes: more visits, then the lower action
    most_visited_step<DPP_XOR1>(best_n, best_a);
    most_visited_step<DPP_XOR2>(best_n, best_a);
    most_visited_step<DPP_HALF_MIRROR>(best_n, best_a);
    return best_n >= 0 ? best_a : -2;
}

// the turn's record: the position before it, valid (1: searched, 4: searched as a fast turn of the playout cap, 2: played
// without a search, 0: no turn), the move
__device__ __forceinline__ void record_turn(const SearchParams &S, const Slot &I, const GameLds &sh, const Game &G, int valid,
                                            int mv, const int (&row_n)[8])
{
    const int64_t row = (int64_t)G.turn * S.games_total + sh.h_game[I.gl];
    if (I.r == 0u) {
        S.rec_own[row] = G.g_own;
        S.rec_opp[row] = G.g_opp;
        S.rec_valid[row] = (uint8_t)valid;
        S.rec_move[row] = (int8_t)(valid ? mv : -1);
    }
#pragma unroll
    for (int i = 0; i < 8; i++)
        S.rec_pi[row * 64 + (int)(8u * I.r) + i] = row_n[i];
}

// MCTS.update_with_move (MCTS.py:149-154): the child of move mv becomes the root, or (no such child) a fresh Node(None, 1.0)
// (one lane)
__device__ __forceinline__ void advance_root(const Tree &T, const Slot &I, uint64_t lg, int rfc, int mv)
{
    int child = -1;
    if (rfc >= 0) {
        if (mv >= 0 && ((lg >> mv) & 1ull))
            child = rfc + __popcll(lg & ((1ull << mv) - 1ull));
        else if (mv == -1 && (int)T.nodes[I.base + rfc].action == -1)
            child = rfc;
    }
    if (child >= 0) {
        T.root[I.g] = child;
        T.nodes[I.base + child].parent = -1;
    } else {
        fresh_root(T, I.g, I.base);
    }
}

// the move mv (< 0: none) on the board, the books, the swap of sides (iago_play_turn; game.py:117-142,253-255); then the
// next turn or the game's end
__device__ __forceinline__ void play_move(const SearchParams &S, const Slot &I, const GameLds &sh, Game &G, bool played, int mv,
                                          const long long t0)
{
    place_stone(G.g_own, G.g_opp, mv, I.L);
    const bool was_over = G.g_over;
    G.stones += played ? 1 : 0;
    const bool passing = !played && !was_over;
    if (passing && G.pass_flg)
        G.stones = 64;                       // a pass after a pass ends the game
    if (!was_over)
        G.pass_flg = passing;
    if (G.turn % 2 == 1)                     // `while stone_num < 64` once per pair of turns
        G.g_over = was_over || G.stones >= 64;
    G.turn++;
    if (G.turn >= S.max_turns || (G.turn % 2 == 0 && G.g_over)) {
        if (I.r == 0u) {
            const int64_t id = sh.h_game[I.gl];
            S.n_turns[id] = G.turn;
            S.game_own[id] = G.g_own;        // (colour 1's stones after an even number of turns)
            S.game_opp[id] = G.g_opp;
        }
        G.state = ST_DONE;
        if (S.trace && I.r == 0u && I.g < S.trace_rows) { // (diagnostic: the game's end, its requests)
            int64_t *row = S.trace + 4 * ((int64_t)S.trace_rows - 1 - I.g);
            row[0] = wall_clock64() - t0;
            row[1] = G.epoch;
            row[2] = G.turn;
        }
    } else {
        G.state = ST_TURN;
    }
}

// ---- 3. whole games (the games' lanes): the turn's end (the move) and the next turn's start, until the game searches
// again or is over (a pass leads straight on to the next turn: at most a few rounds)
// PARK (iago_mcts_search_park): a turn that would be searched at a position of at most S.park_empties empties hands the game
// over instead -- the turn it stands at, its position (own = the mover) and its books, by game id -- and the game is done
// S.explore_turns > 0 (iago_mcts_search_explore): the move of a searched turn below it is the draw from the visit counts
// -- the row the turn records -- keyed by the game's id and its turn
// S.cap_fast > 0 (iago_mcts_search_cap): a turn that searches draws its budget -- S.n_sims playouts, or the first
// S.cap_fast of them (a fast turn: valid 4) -- keyed the same way; the stream stride, the move and the books are untouched
template <bool PARK>
__device__ __forceinline__ void turn_boundary(const SearchParams &S, const iago_row::HwParams &R, const Slot &I, GameLds &sh,
                                              Game &G, const Cursor &C, bool &busy, const long long t0)
{
    const Tree &T = S.T;
    for (int rep = 0; rep < 6; rep++) {
        const bool at_move = G.state == ST_MOVE, at_turn = G.state == ST_TURN, at_draw = G.state == ST_DRAW;
        if (__builtin_amdgcn_ballot_w64(at_move || at_turn || at_draw) == 0ull)
            break;
        busy = busy || at_move || at_turn || at_draw;
        if (at_move || at_turn || at_draw)
            sh.ch_from[I.gl] = -1; // (the root moves, or the tree is a fresh one: the remembered pass chain is void)
        // the turn's Philox word, at ONE call site: explore_word at a turn's end (the draw, below), cap_word at a turn's
        // start -- the budget of the search this turn runs if the mover searches it (a turn that passes or parks leaves a
        // word nobody reads; the 8 lanes write the same word, before the legal set and the root are live)
        const bool explores = S.explore_turns > 0 && at_move && G.turn < S.explore_turns;
        const bool caps = S.cap_fast > 0 && at_turn;
        uint32_t w = 0u;
        if (__builtin_amdgcn_ballot_w64(explores || caps) != 0ull)
            w = turn_word(R.key0, R.key1 ^ (caps ? CAP_KEY : EXPLORE_KEY), R.id_base + (uint32_t)sh.h_game[I.gl], (uint32_t)G.turn);
        if (caps) {
            const bool fast = cap_fast_turn(w, (uint32_t)S.cap_full_256);
            sh.h_budget[I.gl] = fast ? S.cap_fast : S.n_sims;
            sh.h_fast[I.gl] = fast ? 1 : 0;
        }
        const uint64_t lg = group8_legal(to_lane(G.g_own, I.L), to_lane(G.g_opp, I.L), I.L);
        const bool can_move = lg != 0ull && !G.g_over;
        // a match (active 2: PV-MCTS plays colour 1, 3: colour 2; game.py:96-118): the final move when it is the only one
        // is played as it is, by either side (no search, no update_with_move), and the SL policy's turn asks its net for
        // the position and waits to draw
        const int code = (at_turn && can_move && !S.stream) ? (int)S.active[I.g] : 0;
        const bool match = code == 2 || code == 3;
        const bool forced = match && G.stones > 62 && __popcll(lg) == 1;
        const bool policy_turn = match && !forced && (G.turn & 1) == (code == 2 ? 1 : 0);
        if (policy_turn) {
            G.epoch++;
            if (I.r == 0u)
                send_request(S, KIND_POLICY, I.g, G.epoch, G.g_own, G.g_opp); // make_state_var(state, color)
            G.state = ST_WAIT_DRAW;
        }
        bool park = false;
        if constexpr (PARK)
            park = at_turn && can_move && 64 - __popcll(G.g_own | G.g_opp) <= S.park_empties;
        if (park) {
            if (I.r == 0u) {
                const int64_t id = sh.h_game[I.gl];
                S.n_turns[id] = G.turn;
                S.game_own[id] = G.g_own;
                S.game_opp[id] = G.g_opp;
                S.park_stones[id] = G.stones;
                S.park_pass[id] = G.pass_flg ? 1 : 0;
                S.parked[id] = 1;
            }
            G.state = ST_DONE;
        }
        if (at_turn && can_move && !forced && !policy_turn && !park) {
            // the mover searches: MCTS.get_move(state, color) (game.py:112)
            G.n_done = 0;
            if (I.r == 0u)
                S.done[I.g] = G.turn * S.n_sims; // (the rollouts' Philox stream: stream base + turn x n_sims + playout)
            G.state = ST_READY;
        }
        const bool drawn = at_draw || forced; // a stone placed without a search
        const bool moving = at_move || drawn || (at_turn && !can_move);
        const int root = moving ? T.root[I.g] : 0;
        const int rfc = moving ? T.nodes[I.base + root].first_child : -1;
        int row_n[8];
        int best = most_visited(T, I, lg, rfc, at_move, row_n);
        // (once per turn; every lane takes part in the group's sums.  No child visited, or none at all: `best` stays)
        if (__builtin_amdgcn_ballot_w64(explores) != 0ull) {
            const int drawn_a = explore_draw8(row_n, I.r, w);
            best = (explores && drawn_a < 64) ? drawn_a : best;
        }
        if (moving) {
            int mv = -1;
            if (at_move) {
                mv = best;
                if (mv == -2 && I.r == 0u) // max() of an empty children dict (MCTS.py:147): n_sims < n_thr
                    __hip_atomic_store(&S.ctl[CTL_NO_CHILDREN], 1u, RLX_AGENT);
            }
            if (at_draw)
                mv = C.leaf; // the policy's draw
            if (forced)
                mv = (int)__builtin_ctzll(lg); // game.py:97-98
            if (S.rec_move)
                record_turn(S, I, sh, G, at_move ? ((S.cap_fast > 0 && sh.h_fast[I.gl]) ? 4 : 1) : (drawn ? 2 : 0), mv, row_n);
            // for the games not over, and not after a forced final move (game.py:97-98)
            if (!G.g_over && !forced && I.r == 0u)
                advance_root(T, I, lg, rfc, mv);
            play_move(S, I, sh, G, at_move || drawn, mv, t0);
        }
    }
}

// on the way out of a descent that stopped at a node to expand (the games' lanes): ask for its priors and wait.  The node
// WILL expand when they are back, and its children are leaves without a value at their first visits -- the first of them
// in this very playout.  While net workgroups have nothing to do they walk the children's positions beside the policy
// walk, for the position table (nobody waits for these)
__device__ __forceinline__ void ask_priors(const SearchParams &S, const Slot &I, GameLds &sh, Game &G, const Cursor &C)
{
    G.epoch++;
    if (I.r == 0u)
        send_request(S, KIND_POLICY, I.g, G.epoch, C.own, C.opp);
    G.state = ST_WAIT_PRIOR;
    if (sh.pace[3] > 0 && I.need_v) {
        uint64_t rest = group8_legal(to_lane(C.own, I.L), to_lane(C.opp, I.L), I.L);
        while (rest) {
            const int a2 = (int)__builtin_ctzll(rest);
            rest &= rest - 1ull;
            uint64_t c_own = C.own, c_opp = C.opp;
            place_stone(c_own, c_opp, a2, I.L); // the child: the other side moves
            uint32_t known = 0u, by = 0u;
            // (the ring holds QCAP entries: at most one per game that waits -- <= QCAP / 2 games when this is on -- and
            // these, handed out as a budget per workgroup and iteration while the ring was empty, two iterations' worth of
            // which fit beside the games' own: pace[3])
            if (I.r == 0u && !vtable_get(S, c_own, c_opp, known, by) && atomicSub(&sh.pace[3], 1) > 0)
                send_request(S, KIND_VALUE, (int64_t)NOBODY, (uint32_t)I.g, c_own, c_opp); // (reply tag: the sender)
        }
    }
}

// on the way out of a descent that reached the leaf of its playout (MCTS.py:123-127; the games' lanes): its rollout runs
// now, its value is the stored one, the position table's, or is asked for
template <bool WAVE>
__device__ __forceinline__ void reach_leaf(const SearchParams &S, const Slot &I, GameShared<WAVE> &sh, Game &G, Cursor &C,
                                           bool descending)
{
    if (descending && C.fc >= 0 && I.r == 0u)
        S.T.overflow[I.gt] = 1; // path longer than MAX_DEPTH: reported like a full pool
    C.leaf = C.node;
    if constexpr (!WAVE) {
        // the path's final run of pass levels, for the game's next playout -- unless the descent was cut off or the path
        // did not fit its buffer
        if (S.chain_skip && I.r == 0u) {
            const int run = sh.ch_run[I.gl];
            sh.ch_from[I.gl] = (!descending && C.path_n <= S.path_stride && run < C.path_n - 1) ? run : -1;
            sh.ch_len[I.gl] = C.path_n;
        }
    }
    const float c = __uint_as_float(C.vbits);
    C.leaf_fresh = I.need_v && c != c;
    bool ask = C.leaf_fresh;
    if (S.vtable) {
        // has any game of any launch asked for this position before?
        uint32_t hit = 0u, bits = 0u, by = 0u;
        if (C.leaf_fresh && I.r == 0u && vtable_get(S, C.own, C.opp, bits, by)) {
            hit = 1u;
            atomicAdd((unsigned long long *)&S.totals[8], 1ull);
            if (by == (uint32_t)I.g) // (asked for -- or walked ahead -- by this very game)
                atomicAdd((unsigned long long *)&S.totals[12], 1ull);
        }
        hit = group8_add(hit);
        bits = group8_add(I.r == 0u ? bits : 0u);
        if (hit) {
            C.vbits = bits; // (leaf_fresh stays: the backup stores the value in the node)
            ask = false;
        }
    }
    if (ask)
        G.epoch++;
    if (I.r == 0u) {
        S.cur_node[I.g] = C.node;
        S.cur_own[I.g] = C.own;
        S.cur_opp[I.g] = C.opp;
        sh.h_own[I.gl] = C.own; // (what the rollout pass reads)
        sh.h_opp[I.gl] = C.opp;
        sh.h_stream[I.gl] = G.turn * S.n_sims + G.n_done + I.s_in; // (a wave: playout p = the wave's first + the slot)
        if (ask)
            send_request(S, KIND_VALUE, I.g, G.epoch, C.own, C.opp);
    }
    G.state = ask ? ST_ROLL_FRESH : ST_ROLL;
    if constexpr (WAVE) {
        // the playout is in flight: vv + 1 along its path, and the tree's next slot may descend
        __threadfence_block(); // (lane 0's path entries, read by the group's other lanes)
        const int len = C.path_n < S.path_stride ? C.path_n : S.path_stride;
        for (int d = (int)I.r; d < len; d += 8)
            S.T.nodes[I.base + path_entry(I.path_at, I.gpath, d)].reserved1 += 1;
        if (I.r == 0u)
            sh.wv_next[I.tl] = I.s_in + 1;
    }
}

// Node.expand of the cursor node once it has n_thr visits (MCTS.py:109): a pass child or a single legal move without
// a net, else with the priors -- which, when they have not arrived, the descent stops to ask for
// NOISE: the children of the game's ROOT (the path's first node) are created with the mixed priors, from the game's counts
// row (iago_mcts_root_noise wrote it before the launch)
template <int NOISE>
__device__ __forceinline__ void expand(const SearchParams &S, const Slot &I, Cursor &C, bool &descending, bool have_priors,
                                       bool &need_prior)
{
    const Tree &T = S.T;
    const bool grow = descending && C.may_expand && C.fc < 0 && C.nv >= S.n_thr;
    if (__builtin_amdgcn_ballot_w64(grow) == 0ull)
        return;
    const uint64_t lg = group8_legal(to_lane(C.own, I.L), to_lane(C.opp, I.L), I.L);
    if (grow) {
        const int kn = lg ? __popcll(lg) : 1;
        if (lg != 0ull && kn > 1 && !have_priors) {
            need_prior = true; // Node.expand needs policy_func(state) (MCTS.py:118-120)
            descending = false;
        } else {
            C.may_expand = false;
            const uint32_t fc1 = alloc_children(T, I.gt, kn, I.r == 0u);
            if (fc1 != 0u) {
                const int nf = (int)fc1 - 1;
                make_children(T, I.base, nf, C.node, lg, I.r, S.prior_off,
                              [&](int a) { return __uint_as_float(rq::reply_bits(ld(&S.rep_p[I.g * 64 + a]))); });
                if constexpr (NOISE == ROOT_NOISE) {
                    if (C.path_n == 1 && kn > 1) {
                        uint32_t c[8];
#pragma unroll
                        for (int i = 0; i < 8; i++)
                            c[i] = S.noise_counts[I.g * 64 + (int)(8u * I.r) + i];
                        noise_remix_children(T, I.base, nf, lg, I.r, c, (uint32_t)S.noise_eps, (uint32_t)S.noise_lg);
                    }
                }
                if (I.r == 0u)
                    link_children(T, I.base + C.node, nf, kn);
                C.fc = nf;
                C.k = kn;
            }
        }
    }
    __threadfence_block(); // the new children are read by the other lanes of the group below
}

// score_child's sibling under the Gumbel rule: child j of the root, whose record is (s, l), offers its score when it has
// `want` visits; the same strict `>` and the same payload
__device__ __forceinline__ void gumbel_child(const SearchParams &S, const Slot &I, uint4 s, uint4 l, int j, int want, int max_n,
                                             double &best_v, int &best_i, uint32_t (&pl)[4])
{
    const int n = (int)s.x;
    if (n != want)
        return;
    const int a = (int)(int8_t)(l.z & 0xFFu);
    const double v = gumbel_score(S.gumbel_g[I.gt * 64 + (a & 63)], gumbel_logit_q16(__uint_as_float(s.z), S.gumbel_ln),
                                  gumbel_q16(__uint_as_float(s.y), n), max_n, S.gumbel_c_visit, S.gumbel_c_scale);
    if (v > best_v) {
        best_v = v;
        best_i = j;
        pl[0] = l.x, pl[1] = (uint32_t)n, pl[2] = l.z & 0xFFFFu, pl[3] = s.w;
    }
}

// Node.select: two children per lane and step, the argmax over the 8 lanes; the stone; the cursor at the child
// NOISE: at the ROOT of the search (the path's first node) with two or more children a forced child -- mcts_dev.hpp's
// forced_child of its visits, its stored prior and the root's visits, under S.forced_k_256 -- scores +inf
// ROOT_GUMBEL: at the same node the Gumbel rule of iago_hip_serving.h replaces the score: the children whose visit count is
// the schedule's for this playout score g + logit + sigma (mcts_dev.hpp, gumbel_score), every other child -inf
template <bool WAVE, int NOISE>
__device__ __forceinline__ int select_child(const SearchParams &S, const Slot &I, Cursor &C, bool descending)
{
    const int kk = descending ? C.k : 0;
    const double sq = sqrt((double)(WAVE ? C.nv + C.nvv : C.nv));
    const double force_k = (NOISE == ROOT_NOISE && C.path_n == 1 && kk >= 2) ? (double)S.forced_k_256 : 0.0, force_n = (double)C.nv;
    double best_v = -INFINITY;
    int best_i = 0x7fffffff;
    uint32_t pl[4] = {0u, 0u, 0u, 0u};
    // the Gumbel rule's root: t = the children's visits, max_n their largest, `want` the visit count that is served now --
    // the schedule's, or max_n where no child has the schedule's (a root that was not fresh).  Every lane of the group
    // takes part in the three reductions; a game that is not at its root reduces zeros
    [[maybe_unused]] bool groot = false;
    [[maybe_unused]] int want = 0, max_n = 0;
    if constexpr (NOISE == ROOT_GUMBEL) {
        groot = C.path_n == 1 && kk >= 2;
        const int kg = groot ? kk : 0;
        uint32_t t = 0u, mx = 0u;
        for (int j = (int)I.r; j < kg; j += 8) {
            const uint32_t n = (uint32_t)S.T.nodes[I.base + C.fc + j].n_visits;
            t += n;
            mx = max(mx, n);
        }
        t = group8_add(t);
        mx = max(mx, dpp_u32<DPP_XOR1>(mx));
        mx = max(mx, dpp_u32<DPP_XOR2>(mx));
        mx = max(mx, dpp_u32<DPP_HALF_MIRROR>(mx));
        max_n = (int)mx;
        const int row = kk < S.gumbel_m ? kk : S.gumbel_m, col = (int)t < S.n_sims - 1 ? (int)t : S.n_sims - 1;
        want = groot ? (int)S.gumbel_sched[(int64_t)row * S.n_sims + col] : 0;
        uint32_t hit = 0u;
        for (int j = (int)I.r; j < kg; j += 8)
            hit |= S.T.nodes[I.base + C.fc + j].n_visits == want ? 1u : 0u;
        want = group8_add(hit) != 0u ? want : max_n;
    }
    for (int j0 = (int)I.r; j0 < kk; j0 += 16) {
        const int j1 = j0 + 8;
        const bool two = j1 < kk;
        const int64_t c0 = I.base + C.fc + j0, c1 = two ? I.base + C.fc + j1 : c0;
        uint4 s0, l0, s1, l1;
        node_record(S.T, c0, s0, l0);
        node_record(S.T, c1, s1, l1);
        if constexpr (NOISE == ROOT_GUMBEL) {
            if (groot) {
                gumbel_child(S, I, s0, l0, j0, want, max_n, best_v, best_i, pl);
                if (two)
                    gumbel_child(S, I, s1, l1, j1, want, max_n, best_v, best_i, pl);
                continue;
            }
        }
        score_child<WAVE, NOISE == ROOT_NOISE>(S.c_puct, (double)S.vloss, S.visit_off, s0, l0, j0, sq, best_v, best_i, pl, force_k,
                                               force_n);
        if (two)
            score_child<WAVE, NOISE == ROOT_NOISE>(S.c_puct, (double)S.vloss, S.visit_off, s1, l1, j1, sq, best_v, best_i, pl,
                                                   force_k, force_n);
    }
    argmax_step_payload<DPP_XOR1>(best_v, best_i, pl);
    argmax_step_payload<DPP_XOR2>(best_v, best_i, pl);
    argmax_step_payload<DPP_HALF_MIRROR>(best_v, best_i, pl);
    uint64_t own = C.own, opp = C.opp;
    const int action = descending ? (int)(int8_t)(pl[2] & 0xFFu) : -1;
    place_stone(own, opp, action, I.L);
    if (descending) {
        C.own = own;
        C.opp = opp;
        cursor_to<WAVE>(C, C.fc + best_i, pl[0], pl[1], pl[2], pl[2] >> 16, pl[3]);
    }
    return action;
}

// ---- 4. descent (MCTS.py:105-133; the games' lanes): from the root, or on from the leaf whose priors arrived, to a node
// that waits for its priors or to the playout's leaf.  A wave search: one step of its trees' slot order (the slot whose
// turn it is), seeing the in-flight visits and the expansions of the slots before it.  Returns whether the game descended
template <bool WAVE, int NOISE>
__device__ __forceinline__ bool descend(const SearchParams &S, const Slot &I, GameShared<WAVE> &sh, Game &G, Cursor &C,
                                        int pace_limit, int &st_levels, int &st_children)
{
    bool my_turn = true;
    if constexpr (WAVE)
        my_turn = I.s_in == sh.wv_next[I.tl];
    const bool fresh_start = G.state == ST_READY && (WAVE ? my_turn : G.turn * S.n_sims + G.n_done <= pace_limit);
    bool descending = fresh_start || (G.state == ST_PRIOR_READY && my_turn);
    bool have_priors = G.state == ST_PRIOR_READY;
    bool skip_record = G.state == ST_PRIOR_READY; // the cursor node is on the path already
    bool need_prior = false;
    if (fresh_start) {
        const int root = S.T.root[I.gt];
        C.own = I.whole ? G.g_own : S.root_own[I.gt];
        C.opp = I.whole ? G.g_opp : S.root_opp[I.gt];
        uint4 s0, l0;
        node_record(S.T, I.base + root, s0, l0);
        cursor_to<WAVE>(C, root, l0.x, s0.x, l0.z, l0.w, s0.w);
        C.path_n = 0;
        C.may_expand = true;
    }
    // The remembered pass chain (plain search).  A pass child is the only child its parent will ever have and a pass
    // places no stone, so the final run of pass levels of a game's path is the same list of nodes playout after playout
    // -- and the last playout's copy of it is still in the path buffer.  A game that is about to record path index
    // ch_from and stands on the node already there takes the entries up to ch_len - 1 as they are and goes on at the last
    // of them: ONE record instead of one per level (each a round trip to memory, walked in lockstep by the wave's eight
    // games).  Which nodes the path holds, what they count and where the playout ends are the walk's; timing only.
    // jump_at: the path index at which this game may jump (-1: none); jumped: the levels it jumped over in this call, which
    // count against MAX_DEPTH like the walk's (-1: the game ran into that bound after a jump)
    int jump_at = -1, jumped = 0;
    if constexpr (!WAVE) {
        if (S.chain_skip) {
            jump_at = descending ? sh.ch_from[I.gl] : -1;
            if (fresh_start && I.r == 0u)
                sh.ch_run[I.gl] = 0;
        }
    }
    const bool went = descending;
    for (int depth = 0; depth < MAX_DEPTH; depth++) {
        if constexpr (!WAVE) {
            if (descending && depth + jumped >= MAX_DEPTH) { // (the walk's loop would have ended here)
                descending = false;
                jumped = -1;
            }
            if (descending && !skip_record && C.path_n == jump_at) {
                const int len = sh.ch_len[I.gl], n_skip = len - 1 - jump_at;
                const int last = path_entry(I.path_at, I.gpath, len - 1);
                if (path_entry(I.path_at, I.gpath, jump_at) == C.node && depth + n_skip < MAX_DEPTH) {
                    uint4 s0, l0;
                    node_record(S.T, I.base + last, s0, l0);
                    if (n_skip & 1) { // (a pass places nothing; c = 3 - c)
                        const uint64_t t = C.own;
                        C.own = C.opp;
                        C.opp = t;
                    }
                    cursor_to<WAVE>(C, last, l0.x, s0.x, l0.z, l0.w, s0.w);
                    C.path_n = len;
                    skip_record = true; // (the entry is there)
                    jumped = n_skip;
                    st_levels += n_skip; // (the levels of the reference's descent, one child each)
                    st_children += n_skip;
                    if (I.r == 0u)
                        atomicAdd(&sh.wg_count[6], (uint32_t)n_skip);
                }
                jump_at = -1;
            }
        }
        if (descending && !skip_record) {
            if (I.r == 0u) {
                if (C.path_n < S.path_stride) {
                    if (I.path_at >= 0)
                        ((int32_t *)iago_trunk::trunk_lds)[I.path_at + C.path_n] = C.node;
                    else
                        I.gpath[C.path_n] = C.node;
                }
                else
                    S.T.overflow[I.gt] = 1; // deeper than the path buffer: reported like a full pool
            }
            C.path_n++;
        }
        skip_record = false;
        expand<NOISE>(S, I, C, descending, have_priors, need_prior);
        have_priors = false;
        descending = descending && C.fc >= 0; // leaf reached (MCTS.py:107)
        if (__builtin_amdgcn_ballot_w64(descending) == 0ull)
            break;
        st_levels += descending ? 1 : 0;
        st_children += descending ? C.k : 0;
        // Chains of pass nodes.  At the end of a game neither side has a move, and the reference goes on expanding: a pass
        // child under the pass child, one level deeper every n_thr visits (MCTS.py:109-117) -- with 1 .. 3 empties at the
        // root a playout's path is 15 .. 25 nodes long at 100 playouts per move, and 61 % of all levels of a 400-playout
        // game are such levels (LABNOTES.md).  A game that was here in its last playout jumps over them (above); a level
        // that is still walked -- a chain's first playout, a path the last playout did not take -- is this one: a node
        // with ONE child leaves nothing to choose (max over one element, MCTS.py:46), and when that is so for every game
        // of the wave that still descends and all those children are passes, the level is the child's record and the swap
        // of sides, without the scoring
        if (__builtin_amdgcn_ballot_w64(descending && C.k != 1) == 0ull) {
            uint4 s0, l0;
            node_record(S.T, descending ? I.base + C.fc : I.base, s0, l0);
            const bool pass_child = (int)(int8_t)(l0.z & 0xFFu) < 0;
            if (__builtin_amdgcn_ballot_w64(descending && !pass_child) == 0ull) {
                if (descending) {
                    const uint64_t t = C.own; // GameFunctions.place_stone(state, -1, c) places nothing; c = 3 - c
                    C.own = C.opp;
                    C.opp = t;
                    cursor_to<WAVE>(C, C.fc, l0.x, s0.x, l0.z, l0.w, s0.w);
                }
                continue;
            }
        }
        const bool one = C.k == 1;
        const int action = select_child<WAVE, NOISE>(S, I, C, descending);
        if constexpr (!WAVE) {
            // (a step that is no pass level: a pass chain can begin at the child, the next index to be recorded, at the earliest)
            if (S.chain_skip && descending && I.r == 0u && !(one && action < 0))
                sh.ch_run[I.gl] = C.path_n;
        }
    }
    if constexpr (!WAVE)
        descending = descending || jumped < 0;
    if (went) {
        if (need_prior)
            ask_priors(S, I, sh, G, C);
        else
            reach_leaf<WAVE>(S, I, sh, G, C, descending);
    }
    if (I.exists && I.r == 0u)
        S.roll[I.g] = (I.need_z && (G.state == ST_ROLL || G.state == ST_ROLL_FRESH)) ? 1 : 0;
    return went;
}

// ---- 5. the control words this iteration's end looks at (abort, the rings' depths for the pacing and the values-ahead
// gate, the games in play and their progress): eight loads in flight together HERE, under the rollouts -- read one after
// the other by thread 0 between the iteration's last two barriers they were up to six dependent round trips to L2
// (2 - 4 us of a 34 us iteration, with the whole workgroup waiting).  All of it is timing-only state, one iteration old at
// most when it is used.
struct CtlWords {
    uint32_t abort, idle, t0, h0, t1, h1, play, prog, next;
};
__device__ __forceinline__ CtlWords read_ctl(const SearchParams &S, int tid)
{
    CtlWords c = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    if (tid == 0) {
        if (S.stream)
            c.next = __hip_atomic_load(&S.ctl[CTL_NEXT_GAME], RLX_AGENT);
        c.abort = __hip_atomic_load(&S.ctl[CTL_ABORT], RLX_AGENT);
        c.idle = __hip_atomic_load(&S.ctl[CTL_IDLE], RLX_AGENT);
        c.t0 = __hip_atomic_load(&S.ctl[ctl_tail(0)], RLX_AGENT);
        c.h0 = __hip_atomic_load(&S.ctl[ctl_head(0)], RLX_AGENT);
        c.t1 = __hip_atomic_load(&S.ctl[ctl_tail(1)], RLX_AGENT);
        c.h1 = __hip_atomic_load(&S.ctl[ctl_head(1)], RLX_AGENT);
        c.play = __hip_atomic_load(&S.ctl[CTL_PLAYING], RLX_AGENT);
        c.prog = __hip_atomic_load(&S.ctl[CTL_PROGRESS], RLX_AGENT);
    }
    return c;
}

// ---- 6. rollouts of the leaves reached in this iteration (Simulate, mcts_self_play.py:9-134): the games that have one are
// packed into rows of 16 boards (about half of a workgroup's games reach a leaf in an iteration, the others wait for a net:
// one pass of the 16-lanes-per-board body instead of two, most of the time).  A board's game does not depend on its row:
// Philox counters are keyed by the game and its playout count.
// Passes of 16 boards.  A pass costs the same whether it plays 16 boards or one, and all games of the workgroup wait for
// it: when a full pass leaves only a few games over (at most S.roll_defer), they are played in the NEXT iteration's first
// pass, ahead of that iteration's own (17 .. 20 games rolled out in 16 % of the iterations, more than 20 in 32 %:
// LABNOTES.md, round 5).  Timing only: a game's rollout is keyed by its own playout count, whenever it runs.
// Returns whether this game's rollout ran in this iteration (or it needs none)
__device__ __forceinline__ bool rollout_passes(const SearchParams &S, const iago_row::HwParams &R, const Slot &I, GameLds &sh,
                                               bool rolls, bool &deferred, bool &table_ready)
{
    const uint64_t bal = __builtin_amdgcn_ballot_w64(rolls && I.r == 0u); // bit 8 j: game j of this wave
    const uint64_t balo = __builtin_amdgcn_ballot_w64(rolls && deferred && I.r == 0u);
    if ((I.tid & 63) == 0) {
        sh.roll_wave[I.tid >> 6] = (uint32_t)(((bal & 0x0101010101010101ull) * 0x0102040810204080ull) >> 56);
        sh.roll_wave_old[I.tid >> 6] = (uint32_t)(((balo & 0x0101010101010101ull) * 0x0102040810204080ull) >> 56);
    }
    if (I.tid < GAMES_PER_WG)
        sh.roll_list[I.tid] = -1;
    __syncthreads();
    uint32_t gm = 0u, go = 0u; // bit j: game j of the workgroup has a rollout / one put off in the last iteration
#pragma unroll
    for (int w = 0; w < BLOCK / 64; w++) {
        gm |= sh.roll_wave[w] << (8 * w);
        go |= sh.roll_wave_old[w] << (8 * w);
    }
    const int n_roll = __popc(gm), rem = n_roll & 15;
    const int n_now = (n_roll < 16 || rem > S.roll_defer) ? n_roll : n_roll - rem;
    const uint32_t below = (1u << I.gl) - 1u;
    // the games put off last time first, then this iteration's own, each in game order
    const int rank = deferred ? __popc(go & below) : __popc(go) + __popc(gm & ~go & below);
    const bool now = rolls && rank < n_now;
    if (now && I.r == 0u)
        sh.roll_list[rank] = (int32_t)I.g;
    deferred = rolls && !now;
    __syncthreads();
    if (I.tid == 0)
        sh.wg_count[2 + (n_roll == 0 ? 0 : n_roll <= 16 ? 1 : n_roll <= 20 ? 2 : 3)]++; // (diagnostic: totals[10], [13..15])
    const iago_row::RowHandoff hand = {sh.h_own, sh.h_opp, sh.h_stream, sh.h_game, sh.h_z,
                                       (int32_t)((int64_t)I.wg * S.games_per_wg)};
#pragma unroll 1
    for (int at = 0; at < n_now; at += 16) {
        iago_row::rollout_row_body<false, true, true>(R, 0u, sh.roll_list + at, table_ready, &hand);
        table_ready = true;
        __syncthreads();
    }
    return !rolls || now;
}

// ---- 7. a wave search: the backups of every tree whose wave has all its leaf values, in slot order (a step per slot, each
// handing the tree to the next), then the tree's next wave -- or the end of its search
__device__ __forceinline__ void wave_backups(const SearchParams &S, const Slot &I, GameShared<true> &sh, Game &G,
                                             const Cursor &C, const long long c_roll, bool &busy)
{
    const long long c_back = wall_clock64();
    if (I.tid == 0)
        sh.wv_time[1] += c_back - c_roll;
    if (I.mine && I.r == 0u && G.state != ST_HAVE_VALUE && G.state != ST_DONE && I.s_in < sh.wv_size[I.tl])
        sh.wv_block[I.tl] = 1;
    __syncthreads();
    // (a tree in search whose wave blocks nothing: every slot of the wave holds its value, the others are idle)
    const bool ready = I.mine && G.state != ST_DONE && sh.wv_block[I.tl] == 0;
    if (wg_handoff_or(ready)) {
        for (int j = 0; j < I.W; j++) {
            if (ready && I.s_in == j && G.state == ST_HAVE_VALUE) {
                backup_game<true>(S, I.g, I.r, C.leaf, C.leaf_fresh, C.v_reply, C.path_n, sh.h_z[I.gl], sh.negamax, I.path_at, I.gt);
                if (S.trace && I.r == 0u)
                    atomicAdd((unsigned long long *)&S.totals[9], 1ull);
            }
            wg_handoff_or(false);
        }
        if (ready) {
            G.n_done += sh.wv_size[I.tl];
            const int m = S.n_sims - G.n_done < I.W ? S.n_sims - G.n_done : I.W;
            G.state = G.n_done >= S.n_sims ? ST_DONE : (I.s_in < m ? ST_READY : ST_IDLE);
            if (I.r == 0u)
                S.done[I.g] = G.n_done;
            busy = true;
        }
        __syncthreads(); // (every slot has read its tree's wave size)
        if (ready && I.s_in == 0 && I.r == 0u) {
            const int m = S.n_sims - G.n_done < I.W ? S.n_sims - G.n_done : I.W;
            sh.wv_size[I.tl] = m;
            sh.wv_next[I.tl] = 0;
        }
    }
    // (read above, before the barrier: cleared for the next iteration's look)
    if (I.mine && I.r == 0u && I.s_in == 0)
        sh.wv_block[I.tl] = 0;
    if (I.tid == 0)
        sh.wv_time[2] += wall_clock64() - c_back;
}

// ---- 8. the iteration's end: the timeline sample (diagnostic), the pacing books, the clock limit; thread 0 then sets the
// next iteration's pacing limit and values-ahead budget.  Returns whether the launch stops
__device__ __forceinline__ bool iteration_end(const SearchParams &S, const Slot &I, GameLds &sh, const Game &G,
                                              const CtlWords &c, const long long t0, int &contrib, bool &in_play)
{
    const Tree &T = S.T;
    if (S.trace && I.wg == 0 && I.tid == 0 && (int64_t)sh.wg_count[0] < S.trace_rows - T.n_games) {
        const int64_t iters = (int64_t)sh.wg_count[0];
        S.trace[4 * iters + 0] = wall_clock64() - t0;
        S.trace[4 * iters + 1] = __hip_atomic_load(&S.ctl[ctl_tail(0)], RLX_AGENT) + __hip_atomic_load(&S.ctl[ctl_tail(1)], RLX_AGENT);
        S.trace[4 * iters + 2] = __hip_atomic_load(&S.ctl[ctl_head(0)], RLX_AGENT) + __hip_atomic_load(&S.ctl[ctl_head(1)], RLX_AGENT);
        S.trace[4 * iters + 3] = (int64_t)__hip_atomic_load(&S.ctl[CTL_FINISHED], RLX_AGENT) |
                                 (__hip_atomic_load(&S.totals[9], RLX_AGENT) << 8);
    }
    if (I.tid == 0)
        sh.wg_count[0]++;
    const int prog = G.state == ST_DONE ? 0 : G.turn * S.n_sims + G.n_done;
    if (I.mine && I.r == 0u) {
        if (prog != contrib)
            atomicAdd(&sh.pace[0], prog - contrib);
        if (in_play && G.state == ST_DONE)
            atomicAdd(&sh.pace[1], -1);
    }
    contrib = prog;
    in_play = in_play && G.state != ST_DONE;
    // (the workgroup's own stores to done / the tree are read by its next iteration: same CU)
    const bool over = wall_clock64() - t0 > S.clock_limit;
    if (over && I.tid == 0)
        __hip_atomic_store(&S.ctl[CTL_ABORT], 1u, RLX_AGENT);
    const int stop = __syncthreads_or(over || (I.tid == 0 && c.abort != 0u));
    if (I.tid == 0) {
        if (sh.pace[0])
            __hip_atomic_fetch_add(&S.ctl[CTL_PROGRESS], (uint32_t)sh.pace[0], RLX_AGENT);
        if (sh.pace[1])
            __hip_atomic_fetch_add(&S.ctl[CTL_PLAYING], (uint32_t)sh.pace[1], RLX_AGENT);
        sh.pace[0] = 0;
        sh.pace[1] = 0;
        int limit = 0x7fffffff;
        sh.pace[3] = 0;
        const int32_t wait0 = (int32_t)(c.t0 - c.h0), wait1 = (int32_t)(c.t1 - c.h1);
        if (S.ahead_idle >= 0 && S.vtable && I.n_slots <= (int64_t)(QCAP / 2u) && c.idle >= (uint32_t)S.ahead_idle &&
            wait0 <= 0 && wait1 <= 0)
            // this iteration's share of the ring for requests nobody waits for: the games' own requests (at most one
            // each) and TWO iterations' worth of these (the workgroups look at the rings at different moments: a second
            // burst can be on its way before the first shows in anybody's snapshot) fit the ring together
            sh.pace[3] = (int32_t)((QCAP - (uint32_t)I.n_slots) / 2u) / S.n_game_wgs;
        // (a stream: no hold while game ids are left to claim -- the mean then mixes old and new games; the rule
        // holds again for the final drain, when every id is taken)
        if (S.pace_margin >= 0 && (!S.stream || (int64_t)c.next + T.n_games >= (int64_t)S.games_total)) {
            if (wait0 + wait1 > S.pace_backlog && c.play != 0u && c.play <= (uint32_t)T.n_games)
                limit = (int)(c.prog / c.play) + S.pace_margin;
        }
        sh.pace[2] = limit;
    }
    return stop != 0;
}

// ---- 9. a stream whose workgroup has all its games over: its slots take the next block of game ids, one each, and start
// those games together.  (Claimed slot by slot, games of every phase shared a workgroup: a rollout pass lasts as long as
// its longest board and a wave's descent as its deepest game, so every iteration paid for the opening's rollouts AND the
// end's pass chains -- 0.84x / 0.75x the batch loop's games/s at 100 / 400 playouts; LABNOTES.md.)  Which slot plays which
// game changes nothing: a game draws with its own id.  Returns whether the workgroup's games are all over still
__device__ __forceinline__ bool stream_claim(const SearchParams &S, const Slot &I, GameLds &sh, Game &G, bool &in_play)
{
    const Tree &T = S.T;
    const int n_here = (int)min((int64_t)S.games_per_wg, I.n_slots - (int64_t)I.wg * S.games_per_wg); // its slots
    if (I.tid == 0)
        sh.claimed = __hip_atomic_fetch_add(&S.ctl[CTL_NEXT_GAME], (uint32_t)n_here, RLX_AGENT);
    __syncthreads();
    const int64_t next = T.n_games + (int64_t)sh.claimed + I.gl;
    if (I.exists && next < S.games_total) {
        // a fresh tree, except the pool's overflow flag, which voids the launch whichever game set it.  The reply tag
        // `epoch` goes on counting: a reply to the slot's last game is never taken for one to this game
        start_game(G, S.game_own[next], S.game_opp[next]);
        if (I.r == 0u) {
            S.done[I.g] = 0;
            fresh_root(T, I.g, I.base);
            atomicAdd(&sh.pace[1], 1); // (in play again: CTL_PLAYING at the next iteration's end)
        }
        sh.h_game[I.gl] = (int32_t)next;
        sh.ch_from[I.gl] = -1; // (a fresh tree)
        G.state = ST_TURN;
        in_play = true;
    }
    return __syncthreads_and(!I.mine || G.state == ST_DONE) != 0;
}

// ---- 10. after the loop: the descent statistics, the wave timing, the post-mortem of a launch that gave up, the totals
template <bool WAVE>
__device__ __forceinline__ void epilogue(const SearchParams &S, const Slot &I, GameShared<WAVE> &sh, const Game &G,
                                         int st_levels, int st_children, const long long t0)
{
    if (I.exists && I.r == 0u && S.stats) {
        if (WAVE) {
            atomicAdd(&S.stats[2 * I.gt], st_levels);
            atomicAdd(&S.stats[2 * I.gt + 1], st_children);
        } else {
            S.stats[2 * I.g] += st_levels;
            S.stats[2 * I.g + 1] += st_children;
        }
    }
    if constexpr (WAVE) {
        if (I.tid < 4 && S.wave_timing)
            atomicAdd((unsigned long long *)&S.wave_timing[I.tid], (unsigned long long)sh.wv_time[I.tid]);
    }
    // (a launch that gave up: what every unfinished game was waiting for, for the post-mortem -- the trees are void anyway:
    // cur_node = the reply tag it waits for, leaf_value = its state; tools/debug_split_abort.py)
    if (I.exists && I.r == 0u && G.state != ST_DONE && __hip_atomic_load(&S.ctl[CTL_ABORT], RLX_AGENT) != 0u) {
        S.cur_node[I.g] = (int32_t)G.epoch;
        S.leaf_value[I.g] = (float)G.state;
    }
    if (I.tid == 0) {
        atomicAdd((unsigned long long *)&S.totals[2], (unsigned long long)sh.wg_count[0]);
        atomicAdd((unsigned long long *)&S.totals[6], (unsigned long long)sh.wg_count[1]);
        atomicAdd((unsigned long long *)&S.totals[10], (unsigned long long)sh.wg_count[2]);
        atomicAdd((unsigned long long *)&S.totals[13], (unsigned long long)sh.wg_count[3]);
        atomicAdd((unsigned long long *)&S.totals[14], (unsigned long long)sh.wg_count[4]);
        atomicAdd((unsigned long long *)&S.totals[15], (unsigned long long)sh.wg_count[5]);
        if (S.chain_skip) // (a caller that sets the flag gives totals [17])
            atomicAdd((unsigned long long *)&S.totals[16], (unsigned long long)sh.wg_count[6]);
        atomicAdd((unsigned long long *)&S.totals[7], (unsigned long long)(wall_clock64() - t0));
        __hip_atomic_fetch_add(&S.ctl[CTL_FINISHED], 1u, RLX_AGENT);
    }
}

template <bool WAVE, bool PARK = false, int NOISE = ROOT_PLAIN>
__device__ __forceinline__ void game_workgroup(const SearchParams &S, const iago_row::HwParams &R, const long long t0, const int wg)
{
    __shared__ GameShared<WAVE> sh;
    const Slot I = make_slot<WAVE>(S, wg);
    // (a stream: slot g starts game g while there is one -- `active` is not read)
    const bool first = I.exists && I.gt < S.games_total && (S.stream || S.active[I.gt] != 0);
    Game G;
    G.state = (first && S.n_sims > 0) ? (I.whole ? ST_TURN : ST_READY) : ST_DONE;
    G.epoch = 0u;
    if constexpr (WAVE) {
        const int m = S.n_sims < I.W ? S.n_sims : I.W;
        if (G.state == ST_READY && I.s_in >= m)
            G.state = ST_IDLE;
        if (I.tid < GAMES_PER_WG) {
            sh.wv_next[I.tid] = 0;
            sh.wv_size[I.tid] = m;
            sh.wv_block[I.tid] = 0;
        }
        if (I.tid < 4)
            sh.wv_time[I.tid] = 0;
    }
    if (I.exists && I.r == 0u) {
        S.done[I.g] = 0;
        S.roll[I.g] = 0;
    }
    if (I.mine) {
        sh.h_game[I.gl] = (int32_t)I.gt; // (the 8 lanes write the same word; each reads back its own store; a wave: the tree's id)
        sh.h_budget[I.gl] = S.n_sims;    // (every search of the launch, unless a capped turn says otherwise)
        sh.h_fast[I.gl] = 0;
        sh.ch_from[I.gl] = -1; // (no path yet, no remembered pass chain)
    }
    const bool whole_game = I.whole && I.exists && I.g < S.games_total;
    start_game(G, whole_game ? S.game_own[I.g] : 0ull, whole_game ? S.game_opp[I.g] : 0ull);
    if (whole_game && G.state == ST_DONE && I.r == 0u)
        S.n_turns[I.g] = 0;
    Cursor C = {};
    C.fc = -1;
    int st_levels = 0, st_children = 0;
    if (I.tid < 7)
        sh.wg_count[I.tid] = 0u;
    if (I.tid == 7)
        sh.negamax = S.negamax;
    bool deferred = false;    // this game's rollout was put off to the next iteration's first pass
    bool table_ready = false; // the rollout's factor table is in LDS (from the first pass on)
    int contrib = 0;          // pacing: what this game has added to CTL_PROGRESS / whether CTL_PLAYING counts it
    bool in_play = G.state != ST_DONE;
    if (I.tid < 4)
        sh.pace[I.tid] = I.tid == 2 ? 0x7fffffff : 0;
    __syncthreads();
    if (I.mine && in_play && I.r == 0u)
        atomicAdd(&sh.pace[1], 1);
    int pace_limit = 0x7fffffff;

    for (;;) {
        const long long c_it = WAVE ? wall_clock64() : 0;
        bool busy = false; // this game did something in this iteration
        if (I.mine) {
            take_replies(S, R, I, sh, G, C);
            // ---- 2. the backup of a game whose value has arrived (its rollout ran when it descended; a wave search
            // backs its slots up together, below)
            if (!WAVE && G.state == ST_HAVE_VALUE) {
                finish_playout(S, I, sh, G, C, true, C.v_reply);
                busy = true;
            }
            if (!WAVE && I.whole)
                turn_boundary<PARK>(S, R, I, sh, G, C, busy, t0);
        }
        const long long c_desc = WAVE ? wall_clock64() : 0;
        for (int sub = 0; sub < (WAVE ? I.W : 1); sub++) {
            bool went = false;
            if (I.mine) {
                went = descend<WAVE, NOISE>(S, I, sh, G, C, pace_limit, st_levels, st_children);
                busy = busy || went;
            }
            if constexpr (WAVE) {
                if (!wg_handoff_or(went))
                    break;
            }
        }
        if constexpr (WAVE) {
            if (I.tid == 0)
                sh.wv_time[0] += wall_clock64() - c_desc;
        }
        const CtlWords c = read_ctl(S, I.tid);
        const bool rolls = I.mine && I.need_z && (G.state == ST_ROLL || G.state == ST_ROLL_FRESH);
        const long long c_roll = WAVE ? wall_clock64() : 0;
        const bool rolled = rollout_passes(S, R, I, sh, rolls, deferred, table_ready);
        // the leaf's value is at hand (stored or from the table) or -- ROLL_FRESH -- on its way; a wave search's backup
        // waits for the wave's other leaves
        if (I.mine && rolled) {
            if (G.state == ST_ROLL) {
                if constexpr (WAVE) {
                    C.v_reply = __uint_as_float(C.vbits);
                    G.state = ST_HAVE_VALUE;
                } else {
                    finish_playout(S, I, sh, G, C, C.leaf_fresh, __uint_as_float(C.vbits));
                }
            } else if (G.state == ST_ROLL_FRESH) {
                G.state = ST_WAIT_VALUE;
            }
        }
        if constexpr (WAVE)
            wave_backups(S, I, sh, G, C, c_roll, busy);
        const bool stop = iteration_end(S, I, sh, G, c, t0, contrib, in_play);
        bool all_done = __syncthreads_and(!I.mine || G.state == ST_DONE) != 0;
        pace_limit = sh.pace[2];
        if (all_done && !stop && S.stream)
            all_done = stream_claim(S, I, sh, G, in_play);
        if (all_done || stop)
            break;
        if (!__syncthreads_or(busy)) {
            if (I.tid == 0)
                sh.wg_count[1]++;
            __builtin_amdgcn_s_sleep(32); // every game waits for a reply: poll again in ~1 us
            if constexpr (WAVE) {
                if (I.tid == 0)
                    sh.wv_time[3] += wall_clock64() - c_it;
            }
        }
    }
    epilogue<WAVE>(S, I, sh, G, st_levels, st_children, t0);
}

// A NET workgroup: ticket -> entry -> walk -> reply, until every game workgroup has finished.
// The two kinds of net work have a ring each and a HOME on the chip: the workgroups of `policy_xcds` of the 8
// XCDs (workgroup i of a launch runs on XCD i mod 8) serve the POLICY ring, the others the VALUE ring, so that an
// XCD's 4 MB L2 holds ONE net's weights (3.9 / 5.8 MB) instead of thrashing on both; a workgroup whose home ring is
// empty serves the other one (no CU idles while work waits).
// Two VALUE entries that are in the ring together are walked as a PAIR (trunk_item<true, 2>: the two boards
// share the weight stream, which bounds the one-board walk: 46 instead of 70 us of CU time per board; the same
// products in the same order per board: bit-identical values).
//
// net_workgroup is a driver loop over phase functions: the nets' LDS weights, staged once (stage_net_weights) -> per
// item: the claim of a ticket and its entry, or of two (claim) -> the walk and its reply (answer_value, answer_policy)
// -> at the search's end, the counters (leave).  The request's words, the ring's and the mailboxes' granules:
// search_request.hpp; the rings' device functions: beside send_request.

// the workgroup's static LDS: what goes between the claim, the walks and the replies.  (Positions, values and priors
// go between the request's words and the walks through LDS: a store to global memory read back by this very workgroup
// was a round trip to L2, ~2 us under load, twice per walk)
struct NetLds {
    uint32_t req[2][rq::WORDS]; // up to two requests (the low halves of their entries' granules)
    uint32_t status, count;     // the claim's outcome (ring_fetch's status; requests claimed), from wave 0 to all
    float res_v[2], res_p[64];  // a value walk's values, a policy walk's distribution
};
// where the nets' staged weights lie in the dynamic LDS
struct NetWeights {
    float *w1_val, *w1_pol; // block1's weights and biases
    char *head_v;           // the value head (conv_trunk_body.hpp, HEAD_W_*)
    float *head_p;          // conv9 [128], bias10 [64]
};
// what a net workgroup carries from one item to the next
struct NetState {
    // a VALUE ticket taken for a pair whose entry was not there yet: the next round's entry
    uint32_t carry;
    int n_carry;
    u64 *put_e;     // (lanes 0 / 1: the position-table entry whose sequence word is still to be published)
    u64 put_word;
    long long t_wait, t_walk, n_pairs;
};

// ---- 0. both nets' block-1 and head weights into the top of the dynamic LDS, once per workgroup
__device__ __forceinline__ NetWeights stage_net_weights(const iago_trunk::TrunkRParams &VP, const iago_policy::PolicyParams &PP)
{
    const int tid = threadIdx.x;
    // block1's weights and biases of both nets, staged ONCE per workgroup at the top of the dynamic LDS (above the
    // walks' images: conv_trunk_body.hpp, Piece::w1s)
    float *const w1_val = (float *)(iago_trunk::trunk_lds + SEARCH_IMG_TOP), *const w1_pol = w1_val + (64 * 18 + 64);
    for (int e = tid; e < 64 * 18 / 4; e += 256) {
        ((float4 *)w1_val)[e] = ((const float4 *)VP.w1)[e];
        ((float4 *)w1_pol)[e] = ((const float4 *)PP.w1)[e];
    }
    if (tid < 16) {
        ((float4 *)(w1_val + 64 * 18))[tid] = ((const float4 *)VP.b1)[tid];
        ((float4 *)(w1_pol + 64 * 18))[tid] = ((const float4 *)PP.b1)[tid];
    }
    // ... and the heads' weights (the value net's 48.5 KB: block9 as MFMA operand, fc10 transposed so that a thread's row is
    // read at 16 B between threads, fc11, block9's bias; the policy net's conv9 and bias10): read once per walk from
    // global memory they are evicted from L2 by the trunks' weight streams in between
    char *const head_v = (char *)(w1_pol + (64 * 18 + 64));
    float *const head_p = (float *)(head_v + iago_trunk::HEAD_W_LDS);
    for (int e = tid; e < 512; e += 256) {
        ((uint4 *)head_v)[e] = VP.w9_hi[e];
        ((uint4 *)(head_v + iago_trunk::HEAD_W_W9LO))[e] = VP.w9_lo[e];
    }
    for (int e = tid; e < 128 * 16; e += 256) // fc10 [128][64]: row j = e / 16, float4 column c = e % 16
        ((float4 *)(head_v + iago_trunk::HEAD_W_W10))[(e & 15) * 128 + (e >> 4)] = ((const float4 *)VP.w10)[e];
    if (tid < 128)
        ((float *)(head_v + iago_trunk::HEAD_W_W11))[tid] = VP.w11[tid];
    if (tid == 0)
        *(float *)(head_v + iago_trunk::HEAD_W_B9) = VP.b9[0];
    if (tid < 128)
        head_p[tid] = PP.w9[tid];
    if (tid < 64)
        head_p[128 + tid] = PP.b10[tid];
    __syncthreads();
    return NetWeights{w1_val, w1_pol, head_v, head_p};
}

// ---- 1. the claim (wave 0): a ticket and its entry -> L.req[0], and a second VALUE entry -> L.req[1] where
// `pair_backlog` more wait; L.status / L.count for all waves.  In this order: the ticket carried over from the last
// claim, an entry waiting in the home ring, else in the other one; nothing anywhere: poll the counters (no ticket is
// taken for an entry that is not there, so nobody is committed to a ring that stays empty)
__device__ __forceinline__ void claim(const SearchParams &S, const uint32_t home, NetState &N, NetLds &L, const long long t0)
{
    const int tid = threadIdx.x;
    int status = 2, count = 0;
    bool polling = false;
    for (;;) {
        uint32_t q = home;
        bool have = N.n_carry > 0;
        uint32_t t1 = N.carry;
        if (have) {
            q = KIND_VALUE;
            N.n_carry = 0;
        } else if (ring_backlog(S, home) > 0) {
            t1 = ring_take(S, home);
            have = true;
        } else if (ring_backlog(S, home ^ 1u) > 0) {
            q = home ^ 1u;
            t1 = ring_take(S, q);
            have = true;
        }
        if (have) {
            // (a ticket below the tail: its producer is writing the entry right now; one beyond it -- two
            // workgroups saw the same entry -- waits for the next entry of that ring)
            status = ring_fetch(S, q, t1, 0u, L.req[0], t0);
            count = status == 0 ? 1 : 0;
            if (status == 0 && q == KIND_VALUE && ring_backlog(S, KIND_VALUE) >= S.pair_backlog) {
                // (four boards per walk were measured too: the third variant's registers spill in this
                // kernel and the walks lose more than the shared stream gains: LABNOTES.md, round 4)
                const uint32_t t2 = ring_take(S, KIND_VALUE);
                if (ring_fetch(S, KIND_VALUE, t2, 8u, L.req[1], t0) == 0) {
                    count = 2;
                } else {
                    N.carry = t2; // not there yet: the next round's entry
                    N.n_carry = 1;
                }
            }
            break;
        }
        if (search_over(S, t0))
            break; // status 2: every game workgroup is done (no request can come any more), or given up
        if (!polling) {
            polling = true; // (counted while it polls: values ahead of their visit go to idle hands only)
            if (tid == 0)
                __hip_atomic_fetch_add(&S.ctl[CTL_IDLE], 1u, RLX_AGENT);
        }
        __builtin_amdgcn_s_sleep(16);
    }
    if (polling && tid == 0)
        __hip_atomic_fetch_add(&S.ctl[CTL_IDLE], 0xFFFFFFFFu, RLX_AGENT);
    if (tid == 0) {
        L.status = (uint32_t)status;
        L.count = (uint32_t)count;
    }
}

// ---- 2a. a value walk of `count` boards: the values to the games' mailboxes, and into the position table (its first
// step: vtable_put_begin; the driver's next iteration publishes)
__device__ __forceinline__ void answer_value(const SearchParams &S, const iago_trunk::TrunkRParams &VP, NetState &N, NetLds &L,
                                             const NetWeights &Wt, const int64_t row0, const int count)
{
    const int tid = threadIdx.x;
    iago_trunk::Piece W = iago_trunk::whole_walk(VP);
    W.pos = L.req[0];
    W.res = L.res_v;
    W.w1s = Wt.w1_val;
    W.head_w = Wt.head_v;
    if (count == 2)
        iago_trunk::trunk_item<true, 2, true>(VP, W, row0, row0 + count);
    else
        iago_trunk::trunk_item<true, 1, true>(VP, W, row0, row0 + count);
    __syncthreads();
    if (tid < count) {
        const uint32_t *r = L.req[tid];
        const uint32_t bits = __float_as_uint(L.res_v[tid]);
        reply_value(S, r, bits);
        if (S.vtable) // (the writer: the game that asked; nobody: the sender, in the request's tag)
            N.put_e = vtable_put_begin(S, rq::own(r), rq::opp(r), bits, rq::game(r) != NOBODY ? rq::game(r) : rq::tag(r),
                                       N.put_word);
    }
}

// ---- 2b. a policy walk: the distribution to the game's mailbox
__device__ __forceinline__ void answer_policy(const SearchParams &S, const iago_policy::PolicyParams &PP, NetLds &L,
                                              const NetWeights &Wt, const int64_t row0)
{
    const int tid = threadIdx.x;
    iago_policy::policy_item<true>(PP, row0, L.req[0], L.res_p, Wt.w1_pol, Wt.head_p);
    __syncthreads();
    if (tid < 64)
        reply_prior(S, L.req[0], tid, __float_as_uint(L.res_p[tid]));
}

// ---- 3. the search is over: this workgroup's pair walks and its waiting / walking time
__device__ __forceinline__ void leave(const SearchParams &S, const NetState &N)
{
    if (threadIdx.x == 0) {
        atomicAdd((unsigned long long *)&S.totals[3], (unsigned long long)N.n_pairs);
        atomicAdd((unsigned long long *)&S.totals[4], (unsigned long long)N.t_wait);
        atomicAdd((unsigned long long *)&S.totals[5], (unsigned long long)N.t_walk);
    }
}

__device__ __forceinline__ void net_workgroup(const SearchParams &S, const iago_trunk::TrunkRParams &VP,
                                              const iago_policy::PolicyParams &PP, const long long t0, const int wg)
{
    __shared__ __align__(16) NetLds L;
    const int tid = threadIdx.x;
    const int64_t row0 = 4 * (int64_t)wg; // this workgroup's rows of wg_own / wg_opp / out / probs (two in use)
    // the ring it serves first.  (By value, not a field of NetState: as a field the single launch measured 0.35 % slower
    // than the parent, twice; LABNOTES.md, "The net workgroup in named phases")
    const uint32_t home = ((int)((uint32_t)wg & 7u) >= 8 - S.policy_xcds) ? KIND_POLICY : KIND_VALUE;
    NetState N = {0u, 0, nullptr, 0, 0, 0, 0};
    const NetWeights Wt = stage_net_weights(VP, PP);
    for (;;) {
        const long long c0 = wall_clock64();
        if (N.put_e) { // (the last value walk's table entry: vtable_put_begin)
            vtable_put_end(N.put_e, N.put_word);
            N.put_e = nullptr;
        }
        if (tid < 64)
            claim(S, home, N, L, t0); // ticket -> entry
        __syncthreads();
        const long long c1 = wall_clock64();
        N.t_wait += c1 - c0;
        if (L.status != 0u) {
            leave(S, N);
            return;
        }
        const uint32_t kind = rq::kind(L.req[0]);
        const int count = (int)L.count;
        N.n_pairs += count - 1;
        if (kind == KIND_VALUE)
            answer_value(S, VP, N, L, Wt, row0, count); // walk -> reply
        else
            answer_policy(S, PP, L, Wt, row0);
        __syncthreads(); // the next item re-stages the LDS image and the requests
        N.t_walk += wall_clock64() - c1;
    }
}

// ONE grid: the game workgroups first (they are dispatched first, so all of them are resident whatever else
// holds CUs; a net workgroup never waits for another net workgroup, so one that finds no CU free simply starts
// late), then the net workgroups.  A game workgroup whose games are done serves the queue like the others.
template <bool WAVE, bool PARK = false, int NOISE = ROOT_PLAIN>
__device__ __forceinline__ void search_body(const SearchParams &S, const iago_row::HwParams &R, const iago_trunk::TrunkRParams &VP,
                                            const iago_policy::PolicyParams &PP)
{
    const long long t0 = wall_clock64();
    const int wg = (int)blockIdx.x;
    if (wg == 0 && threadIdx.x == 0) // (what the launch was given: the host sized the grid from the device)
        __hip_atomic_store(&S.ctl[CTL_NET_WGS], (uint32_t)gridDim.x - (uint32_t)S.n_game_wgs, RLX_AGENT);
    if (wg < S.n_game_wgs)
        game_workgroup<WAVE, PARK, NOISE>(S, R, t0, wg);
    net_workgroup(S, VP, PP, t0, wg);
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void search_kernel(
    SearchParams S, iago_row::HwParams R, iago_trunk::TrunkRParams VP, iago_policy::PolicyParams PP)
{
    search_body<false>(S, R, VP, PP);
}

// The wave search (iago_mcts_search_wave): the same grid, game workgroups of 32 SLOTS, S.wave of them per tree.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void search_wave_kernel(
    SearchParams S, iago_row::HwParams R, iago_trunk::TrunkRParams VP, iago_policy::PolicyParams PP)
{
    search_body<true>(S, R, VP, PP);
}

// The same search as TWO launches that run together, one per role (iago_mcts_search_split: each on a stream of its own
// whose CU mask gives it CUs no other launch of the process gets -- co-residency by construction, not by a guess of how
// many CUs are free).  Each role is compiled for its own register budget: the game workgroups (VALU and latency: lone
// waves) as a kernel of at most 256 registers, TWO workgroups per CU, so that a wave's waits are another wave's issue
// slots; the net workgroups without the game code in their allocation.  Same device functions, same protocol, same
// trees.  What it buys is CUs: in the single launch every game workgroup holds a CU alone (512 registers per lane), so
// beyond 32 game workgroups each one is a net workgroup less -- 2048 games: 64 + 192 workgroups, 17.1 M leaf-evals/s;
// split: 64 game workgroups on 32 CUs + 224 net workgroups, 18.3 M; 4096 games 10.8 -> 15.1 M; at 1024 games (32 + 224
// either way) the two forms measure the same and the single launch stays (LABNOTES.md, round 6).
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void search_game_kernel(SearchParams S,
                                                                                                   iago_row::HwParams R)
{
    game_workgroup<false>(S, R, wall_clock64(), (int)blockIdx.x);
}

// The whole-game search that hands its games over at park_empties (iago_mcts_search_park): the single launch and the game
// launch of the role split, instantiations of their own -- the kernels above compile the code they always did.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void search_park_kernel(
    SearchParams S, iago_row::HwParams R, iago_trunk::TrunkRParams VP, iago_policy::PolicyParams PP)
{
    search_body<false, true>(S, R, VP, PP);
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void search_game_park_kernel(SearchParams S,
                                                                                                        iago_row::HwParams R)
{
    game_workgroup<false, true>(S, R, wall_clock64(), (int)blockIdx.x);
}

// The search with root noise (iago_mcts_search_noise: one search per launch): again instantiations of their own, for the
// single launch and the role split's game launch.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void search_noise_kernel(
    SearchParams S, iago_row::HwParams R, iago_trunk::TrunkRParams VP, iago_policy::PolicyParams PP)
{
    search_body<false, false, ROOT_NOISE>(S, R, VP, PP);
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void search_game_noise_kernel(SearchParams S,
                                                                                                         iago_row::HwParams R)
{
    game_workgroup<false, false, ROOT_NOISE>(S, R, wall_clock64(), (int)blockIdx.x);
}

// The search under the Gumbel root rule (iago_mcts_search_gumbel: one search per launch): instantiations of their own once
// more, for the single launch and the role split's game launch.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void search_gumbel_kernel(
    SearchParams S, iago_row::HwParams R, iago_trunk::TrunkRParams VP, iago_policy::PolicyParams PP)
{
    search_body<false, false, ROOT_GUMBEL>(S, R, VP, PP);
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void search_game_gumbel_kernel(SearchParams S,
                                                                                                          iago_row::HwParams R)
{
    game_workgroup<false, false, ROOT_GUMBEL>(S, R, wall_clock64(), (int)blockIdx.x);
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void search_net_kernel(
    SearchParams S, iago_trunk::TrunkRParams VP, iago_policy::PolicyParams PP)
{
    const long long t0 = wall_clock64();
    if (blockIdx.x == 0 && threadIdx.x == 0)
        __hip_atomic_store(&S.ctl[CTL_NET_WGS], (uint32_t)gridDim.x, RLX_AGENT);
    net_workgroup(S, VP, PP, t0, (int)blockIdx.x);
}

// The ARENA (iago_mcts_search_arena): TWO searches of the kind above in one grid, each with its own nets, trees, rings
// and constants -- they share the grid and the clock, nothing else.  Agent A's game workgroups come first, then B's
// (all of them dispatched first, as in the single search), then the net workgroups.  A workgroup has a HOME agent:
// a game workgroup its own; a net workgroup the parity of its block index -- workgroup i runs on XCD i mod 8, so the
// even XCDs serve A and the odd ones B, and with the home rings of `policy_xcds` = 2 (XCD 6 / 7: the policy ring) an
// XCD's L2 still holds ONE weight set.  Whoever has nothing left to do for its home agent -- every game workgroup of
// that agent has finished, or it gave up -- serves the other agent's rings to that search's end (net_workgroup's
// prologue restages the other nets' LDS weights).  No net workgroup waits for another, and with two net workgroups
// resident (consecutive block indices: one of each parity) both agents have a server while their games run.
// Both parameter sets are kernel arguments; a workgroup picks its set by a uniform choice on its block index and reads
// it with scalar loads, so there is ONE body of game and net code in the kernel, not two.
struct ArenaSet {
    SearchParams S;
    iago_row::HwParams R;
    iago_trunk::TrunkRParams VP;
    iago_policy::PolicyParams PP;
};
struct ArenaArgs {
    ArenaSet set[2]; // agent A, agent B
};
static_assert(sizeof(ArenaArgs) <= 4096, "the arena's two parameter sets must fit the kernel argument segment");

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void search_arena_kernel(ArenaArgs P)
{
    const long long t0 = wall_clock64();
    const int b = (int)blockIdx.x;
    const int ga = P.set[0].S.n_game_wgs, games = ga + P.set[1].S.n_game_wgs;
    if (b == 0 && threadIdx.x == 0) {
        __hip_atomic_store(&P.set[0].S.ctl[CTL_NET_WGS], (uint32_t)gridDim.x - (uint32_t)games, RLX_AGENT);
        __hip_atomic_store(&P.set[1].S.ctl[CTL_NET_WGS], (uint32_t)gridDim.x - (uint32_t)games, RLX_AGENT);
    }
    const int home = b < games ? (b >= ga ? 1 : 0) : (b & 1);
    if (b < games) {
        const ArenaSet &X = P.set[home];
        game_workgroup<false>(X.S, X.R, t0, home ? b - ga : b);
    }
#pragma unroll 1
    for (int pass = 0; pass < 2; pass++) {
        const ArenaSet &X = P.set[home ^ pass];
        net_workgroup(X.S, X.VP, X.PP, t0, b); // (rows of wg_own / wg_opp by the block index: one owner per row in both agents' arrays)
    }
}

constexpr int search_lds() { return SEARCH_IMG_TOP + iago_trunk::W1_LDS + iago_policy::W1_LDS + iago_trunk::HEAD_W_LDS + 192 * 4; }

// (iago_mcts_search_streams_create: one launch per masked stream of a kernel that needs more scratch memory per lane than
// the game launch does, so that the runtime sizes the streams' scratch ONCE, before any launch that another launch waits
// for: a stream's first dispatch with a private segment is held until the host has allocated it)
__global__ void search_scratch_warm_kernel(uint32_t *out, int n)
{
    volatile uint32_t a[64];
    for (int i = 0; i < 64; i++)
        a[i] = (uint32_t)(i * n) + threadIdx.x;
    uint32_t sum = 0;
    for (int i = 0; i < 64; i++)
        sum += a[(i * 7 + n) & 63];
    if (n == 0x7fffffff && out)
        out[0] = sum;
}

// What the runtime has said of a kernel a search can be launched as.  It is asked once per device (a process may drive
// several): every launch comes through here.
struct FormCache {
    const void *kernel;
    std::atomic<uint64_t> reserved{0}; // devices on which its dynamic LDS is reserved (iago_reserve_lds's bits)
    int static_lds = -1;               // bytes; -1 = not asked yet
    struct {
        int lds = -1, per_cu = 0, cus = 0; // workgroups per CU at `lds` bytes of dynamic LDS (-1 = not asked yet); the
    } on[64];                              // device's CUs, where a caller counts them too (0 = not asked yet)
};

// The variants of a launch, one row each: the entry point's name, its refusal when the single launch's LDS cannot be
// reserved (none: iago_mcts_search_capacity reserves the plain kernel's), the single launch's kernel and the role split's
// game launch's (none: the wave search is not split), each with its books beside it.  The two kernel columns are typed by
// their argument lists: a kernel named in the other column does not compile.
using SearchKernel = void (*)(SearchParams, iago_row::HwParams, iago_trunk::TrunkRParams, iago_policy::PolicyParams);
using GameKernel = void (*)(SearchParams, iago_row::HwParams);
struct Variant {
    const char *who, *no_lds;
    SearchKernel single;
    GameKernel game;
    FormCache single_form{(const void *)single}, game_form{(const void *)game};
};
struct {
    Variant plain, wave, park, noise, gumbel; // (forced playouts: the noise variant)
} variants = {
    {"iago_mcts_search_persistent", nullptr, search_kernel, search_game_kernel},
    {"iago_mcts_search_wave", "iago_mcts_search_wave: cannot reserve the nets' LDS image", search_wave_kernel, nullptr},
    {"iago_mcts_search_park", "iago_mcts_search_park: cannot reserve the nets' LDS image", search_park_kernel, search_game_park_kernel},
    {"iago_mcts_search_noise", "iago_mcts_search_noise: cannot reserve the nets' LDS image", search_noise_kernel, search_game_noise_kernel},
    {"iago_mcts_search_gumbel", "iago_mcts_search_gumbel: cannot reserve the nets' LDS image", search_gumbel_kernel, search_game_gumbel_kernel}};
FormCache net_form{(const void *)search_net_kernel}, arena_form{(const void *)search_arena_kernel};
std::mutex form_cache_mutex; // (static_lds and on[]; `reserved` is iago_reserve_lds's own)

// reserves `bytes` of dynamic LDS for the form on the current device; `who`: the message of a failure
int reserve_lds(FormCache &f, int bytes, const char *who) { return iago_reserve_lds(f.kernel, bytes, f.reserved, who); }

// the form's static LDS; false: the runtime does not answer
bool static_lds_of(FormCache &f, int &bytes)
{
    std::lock_guard<std::mutex> lock(form_cache_mutex);
    hipFuncAttributes fa;
    if (f.static_lds < 0 && hipFuncGetAttributes(&fa, f.kernel) == hipSuccess)
        f.static_lds = (int)fa.sharedSizeBytes;
    bytes = f.static_lds;
    return bytes >= 0;
}

// the form's workgroups per CU of device `dev` at `lds` bytes of dynamic LDS, and the device's CUs where `cus` is given;
// false: the device does not answer.  One answer is kept per device: that for the LDS size asked about last
bool residency_of(FormCache &f, int dev, int lds, int &per_cu, int *cus)
{
    std::lock_guard<std::mutex> lock(form_cache_mutex);
    auto &r = f.on[dev & 63];
    if (cus && r.cus < 1 && hipDeviceGetAttribute(&r.cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) {
        r.cus = 0;
        return false;
    }
    if (r.lds != lds) {
        r.lds = -1;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&r.per_cu, f.kernel, 256, (size_t)lds) != hipSuccess)
            return false;
        r.lds = lds;
    }
    per_cu = r.per_cu;
    if (cus)
        *cus = r.cus;
    return true;
}

} // namespace

extern "C" int iago_mcts_search_capacity(int32_t *cus, int32_t *workgroups_per_cu)
{
    if (!cus || !workgroups_per_cu)
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_capacity: null pointer");
    if (reserve_lds(variants.plain.single_form, search_lds(), "iago_mcts_search_capacity: cannot reserve the nets' LDS image"))
        return IAGO_ERR_HIP;
    int dev = 0, n_cu = 0, per = 0;
    if (hipGetDevice(&dev) != hipSuccess)
        return iago_fail(IAGO_ERR_HIP, "iago_mcts_search_capacity: hipGetDevice failed");
    if (!residency_of(variants.plain.single_form, dev, search_lds(), per, &n_cu))
        return iago_fail(IAGO_ERR_HIP, "iago_mcts_search_capacity: the device does not answer");
    if (n_cu < 1 || per < 1 || per > 255)
        return iago_fail(IAGO_ERR_CAPACITY, "iago_mcts_search_capacity: the search kernel does not fit a CU of this device");
    *cus = n_cu;
    *workgroups_per_cu = per;
    return IAGO_OK;
}

// The CU-masked streams of the role split (iago_mcts_search_streams_create): the game launch's, the net launch's, and
// the events that order both after the caller's stream and the caller's stream after both.
struct iago_search_streams {
    int device;
    int32_t cus, game_cus;
    hipStream_t game, net;
    hipEvent_t ready, game_done, net_done;
};

namespace {
// What an entry point asks of a launch beyond iago_mcts_search_args.  The default is the plain search.
struct LaunchRequest {
    iago_search_streams *streams = nullptr;       // the role split's two launches on these
    const iago_search_wave_args *wave = nullptr;  // the wave search
    const iago_search_park_args *park = nullptr;  // whole games handed over at park_empties
    int explore_turns = 0;                        // turns whose moves are drawn from the visit counts
    int cap_fast = 0, cap_full_256 = 256;         // the playout cap: playouts of a fast turn, full turns in 256
    const iago_root_noise *noise = nullptr;       // root noise: the counts rows applied where a root expands
    int forced_k_256 = 0;                         // forced playouts at the root (with noise): k_256, 0 = none
    const iago_gumbel_root *gumbel = nullptr;     // the Gumbel root rule: tables, schedule, draws and constants
    // the row of `variants` this request is launched as
    Variant &variant() const
    {
        return wave ? variants.wave : gumbel ? variants.gumbel : noise ? variants.noise : park ? variants.park : variants.plain;
    }
};

// games_per_workgroup without its flags (IAGO_SEARCH_CHAIN_SKIP, IAGO_SEARCH_NEGAMAX, IAGO_SEARCH_PUCT_AZ)
constexpr int SEARCH_FLAGS = IAGO_SEARCH_CHAIN_SKIP | IAGO_SEARCH_NEGAMAX | IAGO_SEARCH_PUCT_AZ;
int games_per_wg_of(const iago_mcts_search_args *a)
{
    return a->games_per_workgroup > 0 ? (a->games_per_workgroup & ~SEARCH_FLAGS) : a->games_per_workgroup;
}

// the arguments of a launch (what does not depend on the device)
int check_args(const iago_mcts_search_args *a, const iago_search_wave_args *wv)
{
    if (!a || !a->tree || !a->value || !a->policy || !a->rollout)
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_persistent: null args");
    const iago_mcts_tree *tree = a->tree;
    if (tree->n_games < 1 || tree->capacity < 1 || !tree->nodes || ((uintptr_t)tree->nodes & 31u) || !tree->n_nodes ||
        !tree->root || !tree->overflow || !tree->has_v)
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_persistent: bad tree (the value cache `v` is required)");
    if (tree->n_games > 0x7FFFFFF0ll)
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_persistent: too many games");
    if (!a->active || !a->cur_node || !a->cur_own || !a->cur_opp || !a->path ||
        a->path_stride < 8 || !a->done || !a->roll || !a->leaf_value || !a->q_slots || !a->ctl || !a->rep_v || !a->rep_p ||
        !a->totals || !a->wg_own || !a->wg_opp || ((uintptr_t)a->q_slots & 63u) || ((uintptr_t)a->rep_p & 7u) ||
        ((uintptr_t)a->rep_v & 7u) || ((uintptr_t)a->ctl & 15u))
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_persistent: null or misaligned state array");
    if (a->n_thr < 1 || a->n_sims < 0 || !(a->lmbda >= 0.0f && a->lmbda <= 1.0f) || a->net_workgroups < 1)
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_persistent: n_thr >= 1, n_sims >= 0, 0 <= lmbda <= 1, "
                                           "net_workgroups >= 1 expected");
    if (a->max_turns < 0 || (a->max_turns > 0 && (!a->game_own || !a->game_opp || !a->n_turns)) ||
        (a->max_turns > 0 && a->rec_move && (!a->rec_own || !a->rec_opp || !a->rec_valid || !a->rec_pi)))
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_persistent: whole games (max_turns > 0) need game_own, game_opp, "
                                           "n_turns, and all of rec_own / rec_opp / rec_valid / rec_move / rec_pi or none");
    if (a->games_total < 0 || (a->games_total > 0 && (a->max_turns == 0 || a->n_sims < 1 || a->z_log || a->z_log_rows > 0 ||
                                                      a->trace || a->trace_rows > 0)))
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_persistent: games_total >= 0; a stream (games_total > 0) plays "
                                           "whole games (max_turns > 0, n_sims >= 1), without z_log or trace");
    if (a->max_turns == 0 && (!a->root_own || !a->root_opp))
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_persistent: root_own / root_opp expected");
    if (a->z_log_rows > 0 && (!a->z_log || !a->z_log_n))
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_persistent: z_log needs z_log_n");
    const iago_rollout_args *ro = a->rollout;
    const int64_t n_slots = tree->n_games * (wv ? wv->width : 1); // (a wave search: the slots' arrays)
    if (wv && n_slots > (int64_t)QCAP)
        return iago_fail(IAGO_ERR_CAPACITY, "iago_mcts_search_wave: more slots (n_games x width) than a request ring holds");
    if (ro->n != n_slots || !ro->z || !ro->table || ((uintptr_t)ro->table & 15u) || ro->log_form || ro->trace ||
        ro->uniforms || ro->throughput_hint != 0)
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_persistent: product-form rollout of the n games without "
                                           "trace / uniforms expected");
    const int gpw = games_per_wg_of(a);
    if (!wv && gpw > 0 && gpw != 8 && gpw != 16 && gpw != 24 && gpw != 32)
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_persistent: games_per_workgroup is 0 (= 32), 8, 16 or 32");
    if (a->max_cus < 0)
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_persistent: max_cus < 0");
    if (a->vtable_slots > 0 && (!a->vtable || ((uintptr_t)a->vtable & 31u) || (a->vtable_slots & (a->vtable_slots - 1)) != 0))
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_persistent: vtable must be 32-byte aligned, vtable_slots a "
                                           "power of two");
    return IAGO_OK;
}

struct SearchGrid {
    int gpw;                                 // games (a wave search: slots) per game workgroup
    int chain_skip;                          // IAGO_SEARCH_CHAIN_SKIP of games_per_workgroup
    int negamax;                             // IAGO_SEARCH_NEGAMAX of games_per_workgroup (the wave search has it too)
    int puct_az;                             // IAGO_SEARCH_PUCT_AZ of games_per_workgroup (likewise)
    int64_t n_slots, n_game_wgs, net_wgs, grid;
    int path_lds_cap, game_lds;              // the games' paths in dynamic LDS: bytes a workgroup may use; the game launch's
};

// the games' side of a grid: slots, game workgroups, and the games' recorded paths in the launch's dynamic LDS when
// they fit there (else in the caller's array)
void size_games(const iago_mcts_search_args *a, const iago_search_wave_args *wv, SearchGrid &G)
{
    G.gpw = wv || games_per_wg_of(a) <= 0 ? GAMES_PER_WG : games_per_wg_of(a);
    // (the wave search's descent keeps its in-flight counts per node and walks every level)
    G.chain_skip = (!wv && a->games_per_workgroup > 0 && (a->games_per_workgroup & IAGO_SEARCH_CHAIN_SKIP)) ? 1 : 0;
    G.negamax = (a->games_per_workgroup > 0 && (a->games_per_workgroup & IAGO_SEARCH_NEGAMAX)) ? 1 : 0;
    G.puct_az = (a->games_per_workgroup > 0 && (a->games_per_workgroup & IAGO_SEARCH_PUCT_AZ)) ? 1 : 0;
    G.n_slots = a->tree->n_games * (wv ? wv->width : 1);
    G.n_game_wgs = (G.n_slots + G.gpw - 1) / G.gpw;
    G.path_lds_cap = SEARCH_IMG_TOP;
    G.game_lds = 0;
}

// the CUs a launch may count on: max_cus where it is positive and smaller, else the device's
int cus_to_count_on(int max_cus, int cus) { return max_cus > 0 && max_cus < cus ? max_cus : cus; }

// the nets of a set walk the rows of its wg_own / wg_opp, four per workgroup of the launch's grid; `msg`: the refusal
int check_net_rows(const iago_mcts_search_args *a, int64_t grid, const char *msg)
{
    if (a->value->n < 4 * grid || a->policy->n < 4 * grid || a->value->planes || a->value->index || a->value->n_dev ||
        a->policy->index || a->policy->n_dev || !a->value->own || a->value->own != a->wg_own ||
        a->value->opp != a->wg_opp || a->policy->own != a->wg_own || a->policy->opp != a->wg_opp)
        return iago_fail(IAGO_ERR_INVALID, msg);
    return IAGO_OK;
}

// The grid follows the device: every game workgroup must be resident together with at least one net workgroup (a game
// waits for replies only net workgroups give), and a net workgroup beyond what fits would only start when another one
// ends -- at the end of the launch.  Resident workgroups = CUs the launch may count on (max_cus, else the device's) x
// workgroups of this kernel per CU (its registers and LDS allow one).
int size_grid(const iago_mcts_search_args *a, const LaunchRequest &q, SearchGrid &G)
{
    size_games(a, q.wave, G);
    int32_t cus = 0, per_cu = 0;
    if (const int rc = iago_mcts_search_capacity(&cus, &per_cu))
        return rc;
    int64_t resident = (int64_t)cus_to_count_on(a->max_cus, cus) * per_cu;
    if (const iago_search_streams *sp = q.streams) {
        // Role split: the game launch has sp->game_cus CUs of its own and the net launch all the others.  A game
        // workgroup keeps its paths in LDS when TWO workgroups with them fit a CU (else in the caller's array)
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev != sp->device || sp->cus != cus)
            return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_split: the streams belong to another device");
        if (a->max_cus != 0)
            return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_split: max_cus must be 0 (the split owns the device's CUs)");
        if (!q.variant().game)
            return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_split: this search has no game launch (the wave search is not split)");
        FormCache &game = q.variant().game_form; // (every variant's game launch is an instantiation with books of its own)
        const size_t want = (size_t)G.gpw * (size_t)a->path_stride * 4u;
        int fixed = 0, per_game = 0;
        if (!static_lds_of(game, fixed))
            return iago_fail(IAGO_ERR_HIP, "iago_mcts_search_split: hipFuncGetAttributes failed");
        G.game_lds = (want + (size_t)fixed + 256u) * 2u <= (size_t)160 * 1024u ? (int)want : 0;
        G.path_lds_cap = G.game_lds;
        if (G.game_lds && reserve_lds(game, 96 * 1024, "iago_mcts_search_split: cannot reserve the game workgroups' LDS"))
            return IAGO_ERR_HIP;
        if (!residency_of(game, dev, G.game_lds, per_game, nullptr))
            return iago_fail(IAGO_ERR_HIP, "iago_mcts_search_split: the device does not answer");
        if (G.n_game_wgs > (int64_t)sp->game_cus * per_game)
            return iago_fail(IAGO_ERR_CAPACITY, "iago_mcts_search_split: the game workgroups do not fit the game launch's CUs "
                                                "(more game CUs, fewer games per launch, or the single launch)");
        // The net launch takes at most 7/8 of the device's CUs (224 of 256), whatever the game launch leaves.  Measured, not
        // understood: with 232 .. 240 net workgroups beside a game launch on 16 / 24 CUs, about one batch in 60 froze --
        // the LAST workgroups of the net launch (block index >= 224: exactly those, in every post-mortem) each took a
        // ticket, stopped executing in the same 100 us, and went on the moment the game launch had ended (at its clock
        // limit); with at most 224, 960 batches in a row on the same settings: none (LABNOTES.md, round 6)
        const int64_t net_cus = cus - (sp->game_cus > cus / 8 ? sp->game_cus : cus / 8);
        resident = G.n_game_wgs + net_cus * per_cu;
    }
    if (G.n_game_wgs + 1 > resident)
        return iago_fail(IAGO_ERR_CAPACITY, "iago_mcts_search_persistent: the game workgroups and one net workgroup do not "
                                            "fit the device together (fewer games per launch, or the per-playout launches)");
    G.net_wgs = std::min<int64_t>(a->net_workgroups, resident - G.n_game_wgs);
    G.grid = G.n_game_wgs + G.net_wgs;
    return check_net_rows(a, G.grid, "iago_mcts_search_persistent: the nets read their rows from wg_own / wg_opp "
                                     "(four rows per workgroup of the grid: n >= 4 x (game + net workgroups)), no gather list, no "
                                     "device count");
}

// the kernels' parameters: the arguments, the grid, the request, the tuning knobs of the environment
SearchParams search_params(const iago_mcts_search_args *a, const SearchGrid &G, const LaunchRequest &q)
{
    const iago_search_wave_args *wv = q.wave;
    SearchParams S;
    S.T = *a->tree;
    S.root_own = a->root_own;
    S.root_opp = a->root_opp;
    S.active = a->active;
    S.c_puct = a->c_puct;
    S.lmbda = a->lmbda;
    S.n_thr = a->n_thr;
    S.n_sims = a->n_sims;
    S.n_game_wgs = (int32_t)G.n_game_wgs;
    S.games_per_wg = G.gpw;
    S.cur_node = a->cur_node;
    S.cur_own = a->cur_own;
    S.cur_opp = a->cur_opp;
    S.path = a->path;
    S.path_stride = a->path_stride;
    S.done = a->done;
    S.roll = a->roll;
    S.z = a->rollout->z;
    S.leaf_value = a->leaf_value;
    S.z_log = a->z_log_rows > 0 ? a->z_log : nullptr;
    S.z_log_n = a->z_log_n;
    S.z_log_rows = a->z_log_rows;
    S.q_slots = (u64 *)a->q_slots;
    S.ctl = a->ctl;
    S.rep_v = (u64 *)a->rep_v;
    S.rep_p = (u64 *)a->rep_p;
    S.totals = a->totals;
    S.stats = a->stats;
    S.wg_own = a->wg_own;
    S.wg_opp = a->wg_opp;
    S.clock_limit = (long long)(a->time_limit_ms > 0 ? a->time_limit_ms : 2000) * 100000ll; // wall_clock64: 100 MHz
    // (tuning knob: a pair shares the weight stream -- 46 instead of 70 us of CU time per board -- but takes 92 us:
    // worth it only while entries queue up)
    static const int pair_backlog = [] {
        const char *e = getenv("IAGO_PERSISTENT_PAIR");
        const int v = e ? atoi(e) : 1;
        return v < 1 ? 0x7fffffff : v;
    }();
    S.pair_backlog = pair_backlog;
    // (tuning knob: 27 % of the nets' CU time is the policy net's)
    static const int policy_xcds = [] {
        const char *e = getenv("IAGO_PERSISTENT_POLICY_XCDS");
        const int v = e ? atoi(e) : 2;
        return v < 0 ? 0 : (v > 7 ? 7 : v);
    }();
    S.policy_xcds = policy_xcds;
    // (tuning knob of the pacing: requests that must be waiting for a leader to hold)
    const char *pace_env = getenv("IAGO_PERSISTENT_PACE_BACKLOG"); // (read per launch: the tests vary it)
    S.pace_backlog = pace_env ? atoi(pace_env) : 128;
    // (pacing evens out the games of a batch: the slots of a wave keep their tree's step)
    S.pace_margin = wv ? -1 : a->pace_margin == 0 ? 16 : (a->pace_margin < 0 ? -1 : a->pace_margin);
    // (tuning knob: net workgroups that must poll for values to be walked ahead of their visit; -1 = never)
    const char *ahead_env = getenv("IAGO_PERSISTENT_AHEAD"); // (read per launch: the tests vary it)
    S.ahead_idle = ahead_env ? atoi(ahead_env) : 4;
    // (tuning knob: games that a full pass of 16 rollouts may leave over for the next iteration)
    const char *defer_env = getenv("IAGO_PERSISTENT_ROLL_DEFER"); // (read per launch: the tests vary it)
    S.roll_defer = defer_env ? atoi(defer_env) : 10;
    if (S.roll_defer < 0 || S.roll_defer > 15)
        S.roll_defer = S.roll_defer < 0 ? 0 : 15;
    S.path_lds_cap = G.path_lds_cap;
    S.wave = wv ? wv->width : 1;
    S.vloss = wv ? wv->vloss : 0.0f;
    S.n_slots = G.n_slots;
    S.wave_timing = wv ? wv->timing : nullptr;
    S.max_turns = a->max_turns;
    S.game_own = a->game_own;
    S.game_opp = a->game_opp;
    S.n_turns = a->n_turns;
    S.rec_own = a->rec_own;
    S.rec_opp = a->rec_opp;
    S.rec_valid = a->rec_valid;
    S.rec_move = a->rec_move;
    S.rec_pi = a->rec_pi;
    S.stream = a->games_total > 0 ? 1 : 0;
    S.games_total = a->games_total > 0 ? a->games_total : (int32_t)a->tree->n_games;
    S.vtable = a->vtable_slots > 0 ? (u64 *)a->vtable : nullptr;
    S.vtable_mask = a->vtable_slots > 0 ? (uint32_t)(a->vtable_slots - 1) : 0u;
    S.trace = a->trace_rows > 0 ? a->trace : nullptr;
    S.trace_rows = a->trace_rows;
    S.park_empties = q.park ? q.park->park_empties : -1;
    S.parked = q.park ? q.park->parked : nullptr;
    S.park_stones = q.park ? q.park->stones : nullptr;
    S.park_pass = q.park ? q.park->pass_flg : nullptr;
    S.explore_turns = q.explore_turns;
    S.cap_fast = q.cap_fast;
    S.cap_full_256 = q.cap_full_256;
    S.chain_skip = G.chain_skip;
    S.negamax = G.negamax;
    S.prior_off = G.puct_az ? PRIOR_OFF_ALPHAZERO : PRIOR_OFF_REFERENCE;
    S.visit_off = G.puct_az ? VISIT_OFF_ALPHAZERO : VISIT_OFF_REFERENCE;
    S.noise_counts = q.noise ? q.noise->counts : nullptr;
    S.noise_eps = q.noise ? q.noise->eps_256 : 0;
    S.noise_lg = q.noise ? __builtin_ctz((unsigned)q.noise->draws) : 0;
    S.forced_k_256 = q.noise ? q.forced_k_256 : 0;
    S.gumbel_g = q.gumbel ? q.gumbel->g : nullptr;
    S.gumbel_ln = q.gumbel ? q.gumbel->ln_q16 : nullptr;
    S.gumbel_sched = q.gumbel ? q.gumbel->sched : nullptr;
    S.gumbel_m = q.gumbel ? q.gumbel->m : 0;
    S.gumbel_c_visit = q.gumbel ? q.gumbel->c_visit : 0;
    S.gumbel_c_scale = q.gumbel ? q.gumbel->c_scale_256 : 0;
    return S;
}

// the nets' and the rollouts' parameters of a launch
int net_params(const iago_mcts_search_args *a, iago_trunk::TrunkRParams &VP, iago_policy::PolicyParams &PP, iago_row::HwParams &R)
{
    if (const int rc = iago_trunk::value_params_of(a->value, VP))
        return rc;
    VP.count_lo = 0;
    VP.count_hi = 0x7fffffff;
    if (const int rc = iago_policy::policy_params_of(a->policy, PP))
        return rc;
    R = iago_row::hw_params_of(a->rollout);
    R.own = a->cur_own;
    R.opp = a->cur_opp;
    R.mask = a->roll;
    R.stream_ids = a->done;
    return IAGO_OK;
}

// every polled word starts from zero: the control block, the request ring and the reply mailboxes
int zero_polled(const iago_mcts_search_args *a, int64_t n_slots, void *stream)
{
    if (hipMemsetAsync(a->ctl, 0, 64, (hipStream_t)stream) != hipSuccess ||
        hipMemsetAsync(a->q_slots, 0, (size_t)2 * QCAP * 64, (hipStream_t)stream) != hipSuccess ||
        hipMemsetAsync(a->rep_v, 0, (size_t)n_slots * 8, (hipStream_t)stream) != hipSuccess ||
        hipMemsetAsync(a->rep_p, 0, (size_t)n_slots * 512, (hipStream_t)stream) != hipSuccess)
        return iago_fail(IAGO_ERR_HIP, "iago_mcts_search_persistent: hipMemsetAsync failed");
    return IAGO_OK;
}

// the zeroing of the polled words and the launch: one kernel, or the role split's two on their masked streams
int launch_search(const iago_mcts_search_args *a, void *stream, const LaunchRequest &q, const SearchGrid &G, const SearchParams &S)
{
    iago_trunk::TrunkRParams VP;
    iago_policy::PolicyParams PP;
    iago_row::HwParams R;
    if (const int rc = net_params(a, VP, PP, R))
        return rc;
    constexpr int lds = search_lds();
    if (const int rc = zero_polled(a, G.n_slots, stream))
        return rc;
    const dim3 grid((unsigned)G.grid), block(256);
    iago_search_streams *const sp = q.streams;
    Variant &v = q.variant();
    if (!sp) {
        if (v.no_lds && reserve_lds(v.single_form, lds, v.no_lds))
            return IAGO_ERR_HIP;
        hipLaunchKernelGGL(v.single, grid, block, lds, (hipStream_t)stream, S, R, VP, PP);
        return iago_check_launch(v.who);
    }
    // both launches after everything queued on the caller's stream so far (the zeroing above included), the caller's
    // stream after both.  The game launch first: the net workgroups leave when the game workgroups have finished
    if (reserve_lds(net_form, lds, "iago_mcts_search_split: cannot reserve the nets' LDS image"))
        return IAGO_ERR_HIP;
    if (hipEventRecord(sp->ready, (hipStream_t)stream) != hipSuccess || hipStreamWaitEvent(sp->game, sp->ready, 0) != hipSuccess ||
        hipStreamWaitEvent(sp->net, sp->ready, 0) != hipSuccess)
        return iago_fail(IAGO_ERR_HIP, "iago_mcts_search_split: cannot order the launches after the stream");
    hipLaunchKernelGGL(v.game, dim3((unsigned)G.n_game_wgs), block, G.game_lds, sp->game, S, R);
    int rc = iago_check_launch("iago_mcts_search_split (game launch)");
    if (rc == IAGO_OK) {
        hipLaunchKernelGGL(search_net_kernel, dim3((unsigned)G.net_wgs), block, lds, sp->net, S, VP, PP);
        rc = iago_check_launch("iago_mcts_search_split (net launch)");
    }
    // (also after a failed launch: whatever did start is waited for by the caller's stream)
    if (hipEventRecord(sp->game_done, sp->game) != hipSuccess || hipEventRecord(sp->net_done, sp->net) != hipSuccess ||
        hipStreamWaitEvent((hipStream_t)stream, sp->game_done, 0) != hipSuccess ||
        hipStreamWaitEvent((hipStream_t)stream, sp->net_done, 0) != hipSuccess)
        return iago_fail(IAGO_ERR_HIP, "iago_mcts_search_split: cannot order the stream after the launches");
    return rc;
}

// every launch but the arena's: the checks, the grid, the parameters, the launch
int search_launch(const iago_mcts_search_args *a, void *stream, const LaunchRequest &q)
{
    SearchGrid G;
    if (const int rc = check_args(a, q.wave))
        return rc;
    if (const int rc = size_grid(a, q, G))
        return rc;
    const SearchParams S = search_params(a, G, q);
    if (q.park && hipMemsetAsync(q.park->parked, 0, (size_t)S.games_total, (hipStream_t)stream) != hipSuccess) {
        (void)hipGetLastError();
        return iago_fail(IAGO_ERR_HIP, "iago_mcts_search_park: clearing parked");
    }
    return launch_search(a, stream, q, G, S);
}

// (iago_mcts_search_park) whether `active` [n] holds a match's codes: read where it lies -- host memory as it is, device
// memory through a copy on the stream.  < 0: the copy failed
int has_match_codes(const uint8_t *active, int64_t n, hipStream_t stream)
{
    hipPointerAttribute_t at;
    const bool on_device = hipPointerGetAttributes(&at, active) == hipSuccess &&
                           (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged);
    (void)hipGetLastError();
    std::vector<uint8_t> copy;
    if (on_device) {
        copy.resize((size_t)n);
        if (hipMemcpyAsync(copy.data(), active, (size_t)n, hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess) {
            (void)hipGetLastError();
            return -1;
        }
        active = copy.data();
    }
    for (int64_t i = 0; i < n; i++)
        if (active[i] > 1)
            return 1;
    return 0;
}

// what iago_mcts_search_park and iago_mcts_search_explore ask of a launch that only self-play games may take: whole
// games, and no match codes in `active` (a stream does not read it: every game of it is self-play)
int self_play_only(const iago_mcts_search_args *a, void *stream, const char *who, const char *why)
{
    if (a->max_turns == 0)
        return iago_fail(IAGO_ERR_INVALID, (std::string(who) + ": whole games only (max_turns > 0)").c_str());
    // (before the other arguments are looked at)
    if (a->games_total == 0 && a->active && a->tree && a->tree->n_games >= 1) {
        const int m = has_match_codes(a->active, a->tree->n_games, (hipStream_t)stream);
        if (m < 0)
            return iago_fail(IAGO_ERR_HIP, (std::string(who) + ": cannot read `active`").c_str());
        if (m)
            return iago_fail(IAGO_ERR_INVALID,
                             (std::string(who) + ": match codes in `active` (self-play games only: " + why + ")").c_str());
    }
    return IAGO_OK;
}

// the reserved fields of an option struct
int check_reserved(const int64_t (&reserved)[4], int32_t reserved0, const char *who)
{
    for (int i = 0; i < 4; i++)
        if (reserved[i] != 0 || reserved0 != 0)
            return iago_fail(IAGO_ERR_INVALID, (std::string(who) + ": reserved fields must be 0").c_str());
    return IAGO_OK;
}

// the hand-over's own arguments
int check_park(const iago_search_park_args *pk, const char *who)
{
    const std::string w(who);
    if (!pk->parked || !pk->stones || !pk->pass_flg)
        return iago_fail(IAGO_ERR_INVALID, (w + ": parked, stones and pass_flg expected").c_str());
    if (const int rc = check_reserved(pk->reserved, pk->reserved0, who))
        return rc;
    if (pk->park_empties < 0 || pk->park_empties > IAGO_ENDGAME_MAX_EMPTIES)
        return iago_fail(IAGO_ERR_INVALID, (w + ": park_empties must be in [0, 20]").c_str());
    return IAGO_OK;
}

// iago_mcts_search_explore and iago_mcts_search_cap from the options they share on: explore_turns, a hand-over on the
// same streams, self-play games only (`why`), the launch
int explore_launch(const iago_mcts_search_args *a, void *stream, const LaunchRequest &q, const char *who, const char *why)
{
    const std::string w(who);
    if (q.explore_turns < 0 || q.explore_turns > IAGO_MAX_TURNS)
        return iago_fail(IAGO_ERR_INVALID, (w + ": explore_turns must be in [0, 128]").c_str());
    if (q.park) {
        if (const int rc = check_park(q.park, (w + " (park)").c_str()))
            return rc;
        if (q.park->streams && q.park->streams != q.streams)
            return iago_fail(IAGO_ERR_INVALID, (w + " (park): park->streams must be NULL or `streams`").c_str());
    }
    if (const int rc = self_play_only(a, stream, who, why))
        return rc;
    return search_launch(a, stream, q);
}

// the arena's sets share nothing a search writes: two pointers that are the same array
bool arena_shared(const iago_mcts_search_args *a, const iago_mcts_search_args *b)
{
    const void *pa[] = {a->ctl, a->q_slots, a->rep_v, a->rep_p, a->tree, a->tree->nodes, a->tree->n_nodes, a->tree->root,
                        a->tree->overflow, a->cur_node, a->cur_own, a->cur_opp, a->path, a->done, a->roll, a->leaf_value,
                        a->rollout->z, a->wg_own, a->wg_opp};
    const void *pb[] = {b->ctl, b->q_slots, b->rep_v, b->rep_p, b->tree, b->tree->nodes, b->tree->n_nodes, b->tree->root,
                        b->tree->overflow, b->cur_node, b->cur_own, b->cur_opp, b->path, b->done, b->roll, b->leaf_value,
                        b->rollout->z, b->wg_own, b->wg_opp};
    for (size_t i = 0; i < sizeof(pa) / sizeof(pa[0]); i++)
        if (pa[i] == pb[i])
            return true;
    // (a position table holds ONE value net's values)
    return a->vtable_slots > 0 && b->vtable_slots > 0 && a->vtable == b->vtable;
}
} // namespace

extern "C" int iago_mcts_search_persistent(const iago_mcts_search_args *a, void *stream)
{
    return search_launch(a, stream, LaunchRequest());
}

extern "C" int iago_mcts_search_split(const iago_mcts_search_args *a, iago_search_streams *streams, void *stream)
{
    if (!streams)
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_split: null streams");
    LaunchRequest q;
    q.streams = streams;
    return search_launch(a, stream, q);
}

extern "C" int iago_mcts_search_wave(const iago_mcts_search_args *a, const iago_search_wave_args *w, void *stream)
{
    if (!a || !w)
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_wave: null args");
    if (w->width != 1 && w->width != 8 && w->width != 16 && w->width != 32)
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_wave: width is 1, 8, 16 or 32");
    if (!(w->vloss >= 0.0f && w->vloss <= 3.4028235e38f))
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_wave: vloss >= 0 (finite) expected");
    if (a->max_turns != 0 || a->games_total != 0)
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_wave: one search per launch (max_turns 0, games_total 0): "
                                           "whole games take iago_mcts_search_persistent");
    LaunchRequest q;
    q.wave = w;
    return search_launch(a, stream, q);
}

extern "C" int iago_mcts_search_park(const iago_mcts_search_args *a, const iago_search_park_args *pk, void *stream)
{
    if (!a || !pk)
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_park: null args");
    if (const int rc = check_park(pk, "iago_mcts_search_park"))
        return rc;
    if (const int rc = self_play_only(a, stream, "iago_mcts_search_park",
                                      "a match's policy side needs the net workgroups to its last move"))
        return rc;
    LaunchRequest q;
    q.streams = pk->streams;
    q.park = pk;
    return search_launch(a, stream, q);
}

extern "C" int iago_mcts_search_explore(const iago_mcts_search_args *a, const iago_search_explore_args *ex, void *stream)
{
    if (!a || !ex)
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_explore: null args");
    if (const int rc = check_reserved(ex->reserved, ex->reserved0, "iago_mcts_search_explore"))
        return rc;
    LaunchRequest q;
    q.streams = ex->streams;
    q.park = ex->park;
    q.explore_turns = ex->explore_turns;
    return explore_launch(a, stream, q, "iago_mcts_search_explore", "a match's moves are not drawn from the visit counts");
}

extern "C" int iago_mcts_search_cap(const iago_mcts_search_args *a, const iago_search_cap_args *cap, void *stream)
{
    if (!a || !cap)
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_cap: null args");
    if (const int rc = check_reserved(cap->reserved, cap->reserved0, "iago_mcts_search_cap"))
        return rc;
    if (cap->n_fast < 1 || cap->n_fast > a->n_sims)
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_cap: n_fast must be in [1, n_sims]");
    if (cap->full_per_256 < 1 || cap->full_per_256 > 256)
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_cap: full_per_256 must be in [1, 256]");
    LaunchRequest q;
    q.streams = cap->streams;
    q.park = cap->park;
    q.explore_turns = cap->explore_turns;
    q.cap_fast = cap->n_fast;
    q.cap_full_256 = cap->full_per_256;
    return explore_launch(a, stream, q, "iago_mcts_search_cap", "a match's searches are not capped");
}

extern "C" int iago_mcts_search_noise(const iago_mcts_search_args *a, const iago_search_noise_args *nz, void *stream)
{
    if (!a || !nz)
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_noise: null args");
    if (const int rc = check_reserved(nz->reserved, 0, "iago_mcts_search_noise"))
        return rc;
    if (const int rc = check_root_noise(&nz->noise, "iago_mcts_search_noise"))
        return rc;
    if (a->max_turns != 0 || a->games_total != 0)
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_noise: one search per launch (max_turns 0, games_total 0): whole "
                                           "games with root noise run turn by turn");
    LaunchRequest q;
    q.streams = nz->streams;
    q.noise = &nz->noise;
    return search_launch(a, stream, q);
}

extern "C" int iago_mcts_search_forced(const iago_mcts_search_args *a, const iago_search_forced_args *fz, void *stream)
{
    if (!a || !fz)
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_forced: null args");
    if (const int rc = check_reserved(fz->reserved, fz->reserved0, "iago_mcts_search_forced"))
        return rc;
    if (const int rc = check_root_noise(&fz->noise, "iago_mcts_search_forced"))
        return rc;
    if (fz->k_256 < 1 || fz->k_256 > 4096)
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_forced: k_256 must be in [1, 4096]");
    if (a->max_turns != 0 || a->games_total != 0)
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_forced: one search per launch (max_turns 0, games_total 0): whole "
                                           "games with forced playouts run turn by turn");
    LaunchRequest q;
    q.streams = fz->streams;
    q.noise = &fz->noise;
    q.forced_k_256 = fz->k_256;
    return search_launch(a, stream, q);
}

extern "C" int iago_mcts_search_gumbel(const iago_mcts_search_args *a, const iago_search_gumbel_args *gz, void *stream)
{
    if (!a || !gz)
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_gumbel: null args");
    if (const int rc = check_reserved(gz->reserved, 0, "iago_mcts_search_gumbel"))
        return rc;
    if (const int rc = iago_check_gumbel_root(&gz->gumbel, "iago_mcts_search_gumbel"))
        return rc;
    if (!gz->gumbel.sched)
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_gumbel: null schedule");
    if (a->max_turns != 0 || a->games_total != 0)
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_gumbel: one search per launch (max_turns 0, games_total 0): whole "
                                           "games under the Gumbel rule run turn by turn");
    if (a->n_sims < 1 || a->n_sims > 32767)
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_gumbel: n_sims must be in [1, 32767] (the schedule's columns)");
    if (a->games_per_workgroup <= 0 || !(a->games_per_workgroup & IAGO_SEARCH_NEGAMAX))
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_gumbel: the negamax backup is required (IAGO_SEARCH_NEGAMAX: a root "
                                           "child's Q must be the root mover's value)");
    if (!(a->games_per_workgroup & IAGO_SEARCH_PUCT_AZ))
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_gumbel: the AlphaZero selection is required (IAGO_SEARCH_PUCT_AZ: a "
                                           "child's stored prior must be the policy's p)");
    LaunchRequest q;
    q.streams = gz->streams;
    q.gumbel = &gz->gumbel;
    return search_launch(a, stream, q);
}

// The arena's own rules: two sets that share nothing, no match codes, one clock, and for both agents the rows of the
// WHOLE grid (any workgroup may walk either agent's nets).  The grid is the single search's, summed over the two sets.
extern "C" int iago_mcts_search_arena(const iago_mcts_search_args *a, const iago_mcts_search_args *b, void *stream)
{
    if (!a || !b)
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_arena: null args");
    const iago_mcts_search_args *const set[2] = {a, b};
    for (int i = 0; i < 2; i++) {
        if (set[i]->max_turns != 0 || set[i]->games_total != 0)
            return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_arena: one search per agent and launch (max_turns 0, "
                                               "games_total 0): a game's two trees live in different workgroups");
        if (const int rc = check_args(set[i], nullptr))
            return rc;
        const int m = has_match_codes(set[i]->active, set[i]->tree->n_games, (hipStream_t)stream);
        if (m < 0)
            return iago_fail(IAGO_ERR_HIP, "iago_mcts_search_arena: cannot read `active`");
        if (m)
            return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_arena: match codes in `active` (0 / 1 expected)");
    }
    if (arena_shared(a, b))
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_arena: the two argument sets share a tree, ctl, q_slots, reply "
                                           "or state arrays, or a position table (each agent needs its own)");
    const int want = a->net_workgroups > b->net_workgroups ? a->net_workgroups : b->net_workgroups;
    if (want < 2)
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_arena: net_workgroups >= 2 expected (a server per agent)");
    // the device's CUs are the search kernel's answer, the workgroups per CU the arena kernel's own
    int32_t cus = 0, per_cu = 0;
    if (const int rc = iago_mcts_search_capacity(&cus, &per_cu))
        return rc;
    constexpr int lds = search_lds();
    if (reserve_lds(arena_form, lds, "iago_mcts_search_arena: cannot reserve the nets' LDS image"))
        return IAGO_ERR_HIP;
    int dev = 0, per = 0;
    if (hipGetDevice(&dev) != hipSuccess)
        return iago_fail(IAGO_ERR_HIP, "iago_mcts_search_arena: hipGetDevice failed");
    if (!residency_of(arena_form, dev, lds, per, nullptr))
        return iago_fail(IAGO_ERR_HIP, "iago_mcts_search_arena: the device does not answer");
    if (per < 1)
        return iago_fail(IAGO_ERR_CAPACITY, "iago_mcts_search_arena: the arena kernel does not fit a CU of this device");
    // (the CUs the launch may count on: the smaller positive max_cus of the two sets, else the device's)
    const int64_t resident = (int64_t)cus_to_count_on(b->max_cus, cus_to_count_on(a->max_cus, cus)) * per;
    SearchGrid G[2];
    int64_t games = 0;
    for (int i = 0; i < 2; i++) {
        size_games(set[i], nullptr, G[i]);
        games += G[i].n_game_wgs;
    }
    if (games + 2 > resident)
        return iago_fail(IAGO_ERR_CAPACITY, "iago_mcts_search_arena: both agents' game workgroups and two net workgroups do "
                                            "not fit the device together (fewer games per launch, or one search after the other)");
    const int64_t net_wgs = std::min<int64_t>(want, resident - games);
    const int64_t grid = games + net_wgs;
    ArenaArgs args;
    ArenaSet *const P = args.set;
    for (int i = 0; i < 2; i++) {
        G[i].net_wgs = net_wgs;
        G[i].grid = grid;
        if (const int rc = check_net_rows(set[i], grid,
                                          "iago_mcts_search_arena: each agent's nets read their rows from its wg_own / "
                                          "wg_opp (four rows per workgroup of the WHOLE grid: n >= 4 x (both agents' game "
                                          "workgroups + net workgroups)), no gather list, no device count"))
            return rc;
        P[i].S = search_params(set[i], G[i], LaunchRequest());
        if (const int rc = net_params(set[i], P[i].VP, P[i].PP, P[i].R))
            return rc;
    }
    // one clock for the launch: the larger limit; an agent that gives up says so in its own ctl and the other finishes
    const long long limit = P[0].S.clock_limit > P[1].S.clock_limit ? P[0].S.clock_limit : P[1].S.clock_limit;
    P[0].S.clock_limit = limit;
    P[1].S.clock_limit = limit;
    for (int i = 0; i < 2; i++)
        if (const int rc = zero_polled(set[i], G[i].n_slots, stream))
            return rc;
    hipLaunchKernelGGL(search_arena_kernel, dim3((unsigned)grid), dim3(256), lds, (hipStream_t)stream, args);
    return iago_check_launch("iago_mcts_search_arena");
}

extern "C" int iago_mcts_search_streams_create(int32_t game_cus, iago_search_streams **out)
{
    if (!out)
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_streams_create: null pointer");
    *out = nullptr;
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        return iago_fail(IAGO_ERR_HIP, "iago_mcts_search_streams_create: the device does not answer");
    // (a multiple of 8 from every side: mask bit i is a CU of XCD i mod 8 -- tools/exp_cu_mask.hip --, so both launches
    // get the same number of CUs on every XCD and workgroup i of a launch still runs on XCD i mod 8)
    if (game_cus < 8 || game_cus % 8 != 0 || cus % 8 != 0 || game_cus > cus / 2)
        return iago_fail(IAGO_ERR_INVALID, "iago_mcts_search_streams_create: game_cus is a multiple of 8, at most half the "
                                           "device's CUs");
    uint32_t gm[32] = {0}, nm[32] = {0};
    if (cus > 1024)
        return iago_fail(IAGO_ERR_CAPACITY, "iago_mcts_search_streams_create: more CUs than the mask holds");
    for (int i = 0; i < cus; i++)
        (i < game_cus ? gm : nm)[i / 32] |= 1u << (i % 32);
    iago_search_streams *sp = new iago_search_streams();
    sp->device = dev;
    sp->cus = cus;
    sp->game_cus = game_cus;
    const uint32_t words = (uint32_t)((cus + 31) / 32);
    bool ok = hipExtStreamCreateWithCUMask(&sp->game, words, gm) == hipSuccess;
    ok = ok && hipExtStreamCreateWithCUMask(&sp->net, words, nm) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&sp->ready, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&sp->game_done, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&sp->net_done, hipEventDisableTiming) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(search_scratch_warm_kernel, dim3(1), dim3(64), 0, sp->game, (uint32_t *)nullptr, 1);
        hipLaunchKernelGGL(search_scratch_warm_kernel, dim3(1), dim3(64), 0, sp->net, (uint32_t *)nullptr, 1);
        ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(sp->game) == hipSuccess &&
             hipStreamSynchronize(sp->net) == hipSuccess;
    }
    if (!ok) {
        (void)hipGetLastError();
        iago_mcts_search_streams_destroy(sp);
        return iago_fail(IAGO_ERR_HIP, "iago_mcts_search_streams_create: no CU-masked streams on this device (use the single "
                                       "launch, iago_mcts_search_persistent)");
    }
    *out = sp;
    return IAGO_OK;
}

extern "C" int iago_mcts_search_streams_destroy(iago_search_streams *sp)
{
    if (!sp)
        return IAGO_OK;
    if (sp->game)
        (void)hipStreamDestroy(sp->game);
    if (sp->net)
        (void)hipStreamDestroy(sp->net);
    if (sp->ready)
        (void)hipEventDestroy(sp->ready);
    if (sp->game_done)
        (void)hipEventDestroy(sp->game_done);
    if (sp->net_done)
        (void)hipEventDestroy(sp->net_done);
    delete sp;
    return IAGO_OK;
}
