// lane_search.hpp -- the lane-per-position alpha-beta search that the exact endgame solver (endgame_kernel.hip) and the
// fixed-depth opponent (alphabeta_kernel.hip) share: one LANE PER POSITION runs a negamax alpha-beta depth-first search
// on the rules of othello_lane.hpp with an explicit stack.
//   * the node a lane works on lives in registers (own, opp, the untried moves, alpha, beta, the best value so far);
//     descending pushes it as one FRAME onto the lane's stack in LDS, laid out [level][lane] (own, opp, untried moves
//     and one packed word of alpha / beta / best / pass flag / move tried), returning pops it.  No runtime-indexed
//     register array anywhere: the kernels have no scratch;
//   * a pass pushes no frame: the node swaps the sides and negates the window in place and negates its value when it
//     returns;
//   * one step of the loop is one node entered, one child's value taken back or one leaf valued; lanes that finish a
//     position claim the next one from a counter in ctl, so a wave is not held back by its one deep position;
//   * the root alone differs: every move that could tie the best value with a lower index is searched with a window
//     that keeps that tie exact, so the root's move is the lowest-indexed move reaching the value, whatever the order
//     (the root rule LOWEST; BEST and ALL below also answer the SET of the moves reaching the value);
//   * every lane reads the wall clock once per step: past the limit the launch gives up (ctl[0] = 1).
// What a search is ON comes as a RULES struct (an object: it may carry launch state such as the solver's mode):
//   ROOT                      the root's rule: LOWEST, BEST or ALL (RootRule below)
//   Info                      the type of a frame's packed word (the frame is 24 B + sizeof(Info) per level and lane)
//   NEG_INF, window()         below every value; the root's window is (-window(), window())
//   COUNT_LAST                a node with one level left has one move and is counted directly: the move ends the game
//   LEAF_CHILDREN             the children of a node with one level left are leaves, valued in the parent by leaf()
//   terminal(own, opp)        the value of a finished game for the side `own`
//   leaf(own, opp, SA)        the value of a leaf for its mover (LEAF_CHILDREN only)
//   pick_move(own, opp, moves, levels, SA)   the untried move to search next at a node with `levels` levels left
//   pack(alpha, beta, best, passed, m) / unpack(info, s) -> m   the packed word of a frame
// The root's remaining levels are an argument of the step: the solver's empties, the opponent's depth.
#pragma once
#include "othello_lane.hpp"

namespace iago {
namespace lane {

constexpr int WAVE = 64; // one wave per workgroup: the stack is the wave's own

// ctl words (uint32): what include/iago_hip_serving.h documents, and the claim counter
constexpr int CTL_GAVE_UP = 0;
constexpr int CTL_CLAIM = 1;
constexpr int CTL_REFUSED = 2;
constexpr int CTL_OVERFLOW = 3;

// What the root (unless it passed: then it is a node like any other) answers besides its value.  The move order, the
// window of the root and the first move's search are the same under all three.
//   LOWEST  the lowest-indexed move reaching the value: a later move that could tie it with a lower index is searched
//           with alpha = best - 1, one with a higher index with alpha = best (it must beat best);
//   BEST    the set of the moves reaching the value (Search::best_set): every later move is searched with
//           alpha = best - 1, whatever its index, so a value equal to best comes back exact (fail-soft) and joins the
//           set, a higher one replaces it.  root_move is the set's lowest bit: LOWEST's move;
//   ALL     every move's value: the root's alpha never rises, every move is searched with the root's full window and its
//           value goes to Search::row[move] (one byte per move); best_set is the argmax, root_move its lowest bit.
// A root with one level left under COUNT_LAST: its one move is the set and that move's value the root's.  A root that
// passed or a finished game: the empty set, nothing written to row.
enum RootRule : int { LOWEST = 0, BEST = 1, ALL = 2 };

// (TURN: iago_play_endgame's own, at a turn's start)
enum Phase : uint32_t { CLAIM = 0, ENTER = 1, NEXT = 2, RETURN = 3, DONE = 4, TURN = 5 };

// a lane's search: the node it works on, the value on its way back, the level, the root's books
struct Search {
    uint32_t phase;
    uint64_t own, opp, moves;
    int alpha, beta, best, v;
    int d;
    uint32_t passed;
    int root_move;
    int64_t nodes;
    uint64_t best_set; // BEST, ALL: the root's moves reaching best (LOWEST never reads it: it costs those kernels nothing)
    int8_t *row;       // ALL: where the root's per-move values go, set by whoever begins the search
};

// the wave's stack in LDS, [level][lane]
template <class Rules>
struct Stack {
    static constexpr int FRAME_BYTES = 3 * sizeof(uint64_t) + sizeof(typename Rules::Info);
    uint64_t *own, *opp, *moves;
    typename Rules::Info *info;
    int levels;
};

template <class Rules>
__device__ __forceinline__ Stack<Rules> make_stack(unsigned char *lds, int levels)
{
    Stack<Rules> K;
    K.own = (uint64_t *)lds;
    K.opp = K.own + levels * WAVE;
    K.moves = K.opp + levels * WAVE;
    K.info = (typename Rules::Info *)(K.moves + levels * WAVE);
    K.levels = levels;
    return K;
}

// the root of a new search: (own, opp) with own to move, the window (-window, window)
__device__ __forceinline__ void search_begin(Search &s, uint64_t own, uint64_t opp, int window)
{
    s.own = own;
    s.opp = opp;
    s.d = 0;
    s.alpha = -window;
    s.beta = window;
    s.nodes = 0;
    s.root_move = -1;
    s.best_set = 0ull;
    s.phase = ENTER;
}

// the search is over: v is the root's value, root_move its move (-1: the root passed, -2: the game was over)
__device__ __forceinline__ bool search_done(const Search &s) { return s.phase == RETURN && s.d == 0; }

// the value v of the child reached by move m, back in its parent (the node in s)
template <class Rules>
__device__ __forceinline__ void take_back(Search &s, int m, int v)
{
    if (s.d == 0 && !s.passed) {
        if constexpr (Rules::ROOT == LOWEST) {
            // root: the lowest index among the moves of the best value (the window kept every tie exact)
            if (v > s.best || (v == s.best && m < s.root_move)) {
                s.best = v;
                s.root_move = m;
            }
        } else {
            // root: the set of the moves of the best value (a value equal to best came back exact)
            if constexpr (Rules::ROOT == ALL)
                s.row[m] = (int8_t)v;
            if (v > s.best) {
                s.best = v;
                s.best_set = 1ull << m;
            } else if (v == s.best) {
                s.best_set |= 1ull << m;
            }
            s.root_move = (int)lowest_bit(s.best_set);
        }
    } else {
        s.best = max(s.best, v);
        s.alpha = max(s.alpha, s.best);
        if (s.alpha >= s.beta)
            s.moves = 0ull; // cut-off
    }
}

// the move of `moves` (not empty) with the fewest replies for the opponent (fastest first; ties: lowest index)
__device__ __forceinline__ uint32_t fewest_replies(uint64_t own, uint64_t opp, uint64_t moves, const ShiftAmounts &SA)
{
    uint32_t best_m = lowest_bit(moves), best_mob = 65u;
    while (moves) {
        const uint32_t m = lowest_bit(moves);
        moves &= moves - 1ull;
        const uint64_t f = flips_of(own, opp, m);
        const uint32_t mob = (uint32_t)__popcll(legal_of(opp & ~f, own | f | (1ull << m), SA));
        if (mob < best_mob) {
            best_mob = mob;
            best_m = m;
        }
    }
    return best_m;
}

// One step of a lane that is searching (phase ENTER, NEXT or RETURN below the root; any other phase: nothing): one node
// entered, one child's value taken back, or one leaf valued.  levels0: the root's remaining levels.  false: the stack
// would overflow (cannot happen: a frame is pushed by a node with at least 2 levels left, levels 0 .. levels0 - 2) --
// nothing was written past it, the caller drops the position.
template <class Rules>
__device__ __forceinline__ bool search_step(Search &s, const Stack<Rules> &K, uint32_t lane, int levels0, const Rules &R,
                                            const ShiftAmounts &SA)
{
    if (s.phase == ENTER) {
        s.nodes++;
        s.passed = 0u;
        uint64_t legal = legal_of(s.own, s.opp, SA);
        if (legal == 0ull) {
            const uint64_t other = legal_of(s.opp, s.own, SA);
            if (other == 0ull) { // neither side can move: the game is over
                s.v = R.terminal(s.own, s.opp);
                if (s.d == 0)
                    s.root_move = -2;
                s.phase = RETURN;
            } else { // pass in place
                const uint64_t t = s.own;
                s.own = s.opp;
                s.opp = t;
                const int a = s.alpha;
                s.alpha = -s.beta;
                s.beta = -a;
                s.passed = 1u;
                legal = other;
            }
        }
        if (s.phase == ENTER) {
            if (Rules::COUNT_LAST && levels0 - s.d == 1) { // the last level: its move ends the game
                const uint32_t m = lowest_bit(legal);
                const uint64_t f = flips_of(s.own, s.opp, m);
                s.nodes++;
                s.v = R.terminal(s.own | f | (1ull << m), s.opp & ~f);
                if (s.passed)
                    s.v = -s.v;
                if (s.d == 0) {
                    s.root_move = s.passed ? -1 : (int)m;
                    if constexpr (Rules::ROOT != LOWEST) {
                        if (!s.passed) {
                            s.best_set = 1ull << m;
                            if constexpr (Rules::ROOT == ALL)
                                s.row[m] = (int8_t)s.v;
                        }
                    }
                }
                s.phase = RETURN;
            } else {
                s.moves = legal;
                s.best = Rules::NEG_INF;
                if (s.d == 0)
                    s.root_move = s.passed ? -1 : 64; // 64: no move yet (above every index)
                s.phase = NEXT;
            }
        }
    } else if (s.phase == RETURN && s.d > 0) {
        // the child's value, back in the parent
        s.d--;
        const int k = s.d * WAVE + (int)lane;
        s.own = K.own[k];
        s.opp = K.opp[k];
        s.moves = K.moves[k];
        const int m = Rules::unpack(K.info[k], s);
        take_back<Rules>(s, m, -s.v);
        s.phase = NEXT;
    }

    if (s.phase == NEXT) {
        const bool root = s.d == 0 && !s.passed;
        const int levels = levels0 - s.d;
        uint32_t m = 0u;
        int a_child = s.alpha;
        bool go = false;
        while (s.moves != 0ull) {
            m = R.pick_move(s.own, s.opp, s.moves, levels, SA);
            s.moves &= ~(1ull << m);
            if constexpr (Rules::ROOT == LOWEST) {
                if (root && s.best > Rules::NEG_INF) // a tie of a lower index must come back exact, a higher one must beat best
                    a_child = max(s.alpha, (int)m < s.root_move ? s.best - 1 : s.best);
            } else if constexpr (Rules::ROOT == BEST) {
                if (root && s.best > Rules::NEG_INF) // every tie must come back exact
                    a_child = max(s.alpha, s.best - 1);
            }
            if (a_child < s.beta) {
                go = true;
                break;
            }
        }
        if (go) {
            const uint64_t f = flips_of(s.own, s.opp, m);
            const uint64_t cown = s.opp & ~f, copp = s.own | f | (1ull << m);
            if constexpr (Rules::LEAF_CHILDREN) {
                if (levels <= 1) { // a child with no level left: a leaf, valued here without a frame
                    s.nodes++;
                    take_back<Rules>(s, (int)m, -R.leaf(cown, copp, SA));
                    return true;
                }
            }
            if (s.d >= K.levels) // cannot happen (d <= levels0 - 2): never write past the stack
                return false;
            const int k = s.d * WAVE + (int)lane;
            K.own[k] = s.own;
            K.opp[k] = s.opp;
            K.moves[k] = s.moves;
            K.info[k] = Rules::pack(s.alpha, s.beta, s.best, s.passed, m);
            s.own = cown;
            s.opp = copp;
            s.alpha = -s.beta;
            s.beta = -a_child;
            s.d++;
            s.phase = ENTER;
        } else {
            s.v = s.passed ? -s.best : s.best;
            s.phase = RETURN;
        }
    }
    return true;
}

// The search of a wave, lane per position, over the indices below n.  P, the kernel's params: ctl, levels (stack frames
// per lane), clock_limit (wall_clock64 ticks), and how an index becomes a search and an answer --
//   admit(pos, own, opp, levels0) -> true: search (own, opp) with levels0 levels; false: refused (counted and answered)
//   finish(pos, s): the outputs of the finished search s;
//   row(pos) (Rules::ROOT == ALL only): where the per-move values of the root go, 64 bytes.
// levels0 comes in as the launch's own where every position has the same (admit leaves it), else as 0.

// What every such params struct holds (lane_host.hpp's fill_lane_params fills it): a kernel's own derives from it and adds
// admit() and the one or two fields that admit() reads.  Score: the type of a value in memory.
template <class Score>
struct LaneParams {
    const uint64_t *own;
    const uint64_t *opp;
    Score *score;
    int8_t *move;
    int64_t *nodes;
    uint8_t *done;
    uint32_t *ctl;
    int32_t levels;          // stack frames per lane
    long long clock_limit;   // wall_clock64 ticks

    // admit()'s false: counted, answered with zeros, the done flag stays 0
    __device__ __forceinline__ bool refuse(int64_t pos) const
    {
        atomicAdd(&ctl[CTL_REFUSED], 1u);
        score[pos] = 0;
        move[pos] = 0;
        nodes[pos] = 0;
        return false;
    }

    __device__ __forceinline__ void finish(int64_t pos, const Search &s) const
    {
        score[pos] = (Score)s.v;
        move[pos] = (int8_t)s.root_move;
        nodes[pos] = s.nodes;
        done[pos] = 1;
    }
};

template <class Rules, class Params>
__device__ __forceinline__ void search_wave(const Params &P, const Rules &R, int64_t n, int levels0,
                                            unsigned char *stack_lds)
{
    const uint32_t lane = threadIdx.x;
    const Stack<Rules> K = make_stack<Rules>(stack_lds, P.levels);
    const ShiftAmounts SA = opaque_shift_amounts();
    const long long t0 = wall_clock64();

    Search s = {};
    s.phase = CLAIM;
    int64_t pos = 0;

    while (true) {
        if (s.phase == CLAIM) {
            if (__hip_atomic_load(&P.ctl[CTL_GAVE_UP], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {
                s.phase = DONE;
            } else {
                pos = (int64_t)atomicAdd(&P.ctl[CTL_CLAIM], 1u);
                uint64_t own, opp;
                if (pos >= n)
                    s.phase = DONE;
                else if (P.admit(pos, own, opp, levels0)) {
                    search_begin(s, own, opp, R.window());
                    if constexpr (Rules::ROOT == ALL)
                        s.row = P.row(pos);
                }
            }
        }
        if (__builtin_amdgcn_ballot_w64(s.phase != DONE) == 0ull)
            break;
        if (wall_clock64() - t0 > P.clock_limit) {
            // give up: what is unfinished keeps its done flag 0 (cleared before the launch)
            if (s.phase != DONE)
                __hip_atomic_store(&P.ctl[CTL_GAVE_UP], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            break;
        }

        if (!search_step(s, K, lane, levels0, R, SA)) {
            atomicOr(&P.ctl[CTL_OVERFLOW], 1u);
            s.phase = CLAIM;
            continue;
        }

        if (search_done(s)) {
            P.finish(pos, s);
            s.phase = CLAIM;
        }
    }
}

} // namespace lane
} // namespace iago
