// lane_host.hpp -- the HOST layer of the lane searches' entry points (endgame_kernel.hip, alphabeta_kernel.hip), stated
// once: how they refuse an argument set, the range checks they share with their texts, the kernel params every search
// kernel takes, and the three stages of a split launch.  An entry point names itself once (`who`) and is its own
// range checks, its rules / Kind, its params and one call; the order of the checks is the entry point's own:
// null / n, its own fields, max_empties, time_limit_ms, the job arrays, the outputs, reserved.
#pragma once
#include "abi_common.hpp"
#include "lane_search.hpp"
#include "lane_split.hpp"

#include "../../include/iago_hip_serving.h"

#include <stdio.h>

namespace iago {
namespace lane {

static_assert(IAGO_OK == 0, "`if (const int rc = check(...)) return rc;` below and in the entry points");

// "<who>: <text>" as the thread's last error
inline int fail(int code, const char *who, const char *text)
{
    char msg[256];
    snprintf(msg, sizeof msg, "%s: %s", who, text);
    return iago_fail(code, msg);
}

inline int refuse(const char *who, const char *text) { return fail(IAGO_ERR_INVALID, who, text); }

// ---- the range checks more than one entry point makes: IAGO_OK, or the refusal

inline int check_mode(const char *who, int32_t mode)
{
    if (mode != IAGO_ENDGAME_EXACT && mode != IAGO_ENDGAME_WLD)
        return refuse(who, "mode must be IAGO_ENDGAME_EXACT or IAGO_ENDGAME_WLD");
    return IAGO_OK;
}

inline int check_max_empties(const char *who, int32_t max_empties)
{
    if (max_empties < 0 || max_empties > IAGO_ENDGAME_MAX_EMPTIES)
        return refuse(who, "max_empties must be in [0, 20]");
    return IAGO_OK;
}

inline int check_time_limit(const char *who, int32_t time_limit_ms)
{
    if (time_limit_ms <= 0 || time_limit_ms > IAGO_ENDGAME_MAX_TIME_MS)
        return refuse(who, "time_limit_ms must be in [1, 600000]");
    return IAGO_OK;
}

inline int check_reserved(const char *who, const int64_t (&reserved)[4], int32_t reserved0 = 0)
{
    if (reserved[0] != 0 || reserved[1] != 0 || reserved[2] != 0 || reserved[3] != 0 || reserved0 != 0)
        return refuse(who, "reserved fields must be 0");
    return IAGO_OK;
}

// time_limit_ms in the ticks of wall_clock64: 100 MHz
inline long long clock_limit_of(int32_t time_limit_ms) { return (long long)time_limit_ms * 100000ll; }

// every cell of the solver's per-move values starts as "no move": the legal moves of the roots answered are written
inline int clear_move_score(const char *who, int8_t *move_score, int64_t n, hipStream_t s)
{
    if (hipMemsetAsync(move_score, IAGO_ENDGAME_NO_MOVE & 0xFF, (size_t)n * 64, s) != hipSuccess) {
        (void)hipGetLastError();
        return fail(IAGO_ERR_HIP, who, "clearing move_score");
    }
    return IAGO_OK;
}

// The fields of a search kernel's params that every search has (LaneParams, lane_search.hpp), over the positions and the
// outputs given; what the kernel's own struct adds is its entry point's to fill.
template <class Score>
void fill_lane_params(LaneParams<Score> &p, const uint64_t *own, const uint64_t *opp, Score *score, int8_t *move,
                      int64_t *nodes, uint8_t *done, uint32_t *ctl, int levels, int32_t time_limit_ms)
{
    p.own = own;
    p.opp = opp;
    p.score = score;
    p.move = move;
    p.nodes = nodes;
    p.done = done;
    p.ctl = ctl;
    p.levels = levels;
    p.clock_limit = clock_limit_of(time_limit_ms);
}

// the positions and the outputs of an unsplit search, over its argument structs; `done`: the struct's done flag,
// further: whether the outputs of the entry point's own are given
template <class Args>
int check_roots(const char *who, const Args *a, const uint8_t *done, bool further = true)
{
    if (a->n < 0 || (a->n > 0 && (!a->own || !a->opp || !a->score || !a->move || !a->nodes || !done || !further)) ||
        !a->ctl)
        return refuse(who, "null pointer or negative n");
    return IAGO_OK;
}

// The clears and the launch of an unsplit search on stream s: `kernel` on its params P (ctl, levels), a lane per index
// below n; move_score: the per-move values to clear first, or null
template <class P>
int lane_run(const char *who, P &p, uint8_t *done, const char *done_name, int64_t n, int8_t *move_score,
             const void *kernel, int frame_bytes, hipStream_t s)
{
    int cus = 0;
    int rc = iago_search_prepare(who, p.ctl, 4, done, done_name, n, s, &cus);
    if (rc != IAGO_OK || cus == 0)
        return rc;
    if (move_score && (rc = clear_move_score(who, move_score, n, s)) != IAGO_OK)
        return rc;
    iago_search_launch(kernel, &p, p.levels, frame_bytes, n, cus, s);
    return iago_check_launch(who);
}

// ---- the split entry points, over their two argument structs (the shared fields have the same names); `done`: the
// roots' done flag, which the solver's struct calls solved

template <class Args>
int split_check_roots(const char *who, const Args *a)
{
    if (a->n < 0 || a->n > INT32_MAX || (a->n > 0 && (!a->own || !a->opp || !a->job_count || !a->job_first)) || !a->ctl)
        return refuse(who, "null pointer, negative n or n above 2^31 - 1");
    return IAGO_OK;
}

// job_capacity, the job arrays (*count_only: all null) and the outputs of the full form
template <class Args>
int split_check_jobs(const char *who, const Args *a, const uint8_t *done, const char *done_name, bool *count_only)
{
    if (a->job_capacity < 0 || a->job_capacity > INT32_MAX)
        return refuse(who, "job_capacity must be in [0, 2^31 - 1]");
    const int job_arrays = (a->job_own != nullptr) + (a->job_opp != nullptr) + (a->job_root != nullptr) +
                           (a->job_path != nullptr) + (a->job_score != nullptr) + (a->job_move != nullptr) +
                           (a->job_nodes != nullptr) + (a->job_done != nullptr);
    if ((job_arrays != 0 && job_arrays != 8) || (job_arrays == 0 && a->job_capacity != 0))
        return refuse(who, "the job arrays are all given, or all null with job_capacity 0 (the count-only form)");
    *count_only = job_arrays == 0;
    if (!*count_only && a->n > 0 && (!a->score || !a->move || !a->nodes || !done)) {
        char text[64];
        snprintf(text, sizeof text, "null score, move, nodes or %s", done_name);
        return refuse(who, text);
    }
    return IAGO_OK;
}

// The stages of lane_split.hpp on the caller's stream: the clears, 1. expand (a count-only call returns there),
// 2. jobs_kernel -- the lanes of the unsplit search -- over the jobs, a stack of `levels` frames each (the deepest job is
// a root that must pass), 3. reduce.  J: jobs_kernel's params with the fields of its own filled.  Kind::MOVES: the
// arguments have best and move_score, which the reduction answers where they are given.
template <class Kind, class Jobs, class Args>
int split_run(const char *who, const Args *a, bool count_only, uint8_t *done, const char *done_name, const Kind &kind,
              const void *jobs_kernel, Jobs J, int levels, int frame_bytes, hipStream_t s)
{
    int cus = 0;
    int rc = iago_search_prepare(who, a->ctl, SPLIT_CTL_WORDS, count_only ? nullptr : done, done_name, a->n, s, &cus);
    if (rc != IAGO_OK || cus == 0)
        return rc;
    if constexpr (Kind::MOVES) {
        if (!count_only && a->move_score && (rc = clear_move_score(who, a->move_score, a->n, s)) != IAGO_OK)
            return rc;
    }

    split_expand(split_params_of(a, kind), count_only, s);
    if (count_only)
        return iago_check_launch(who);

    fill_lane_params(J, a->job_own, a->job_opp, a->job_score, a->job_move, a->job_nodes, a->job_done, a->ctl, levels,
                     a->time_limit_ms);
    iago_search_launch(jobs_kernel, &J, levels, frame_bytes, a->job_capacity, cus, s);

    split_reduce(reduce_params_of<Kind>(a, done), s);
    return iago_check_launch(who);
}

} // namespace lane
} // namespace iago
