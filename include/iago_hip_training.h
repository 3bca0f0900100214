/*
 * iago_hip_training.h -- training the nets on the library's own kernels: the supervised update of the Value net
 * (train_value.py), SLPolicy on the search's visit counts, minibatches out of a replay window of self-play rows, and
 * that window merged by position up to the board's symmetries.  Same conventions as iago_hip.h; part of the library's
 * ABI (iago_abi_version).
 */
#ifndef IAGO_HIP_TRAINING_H
#define IAGO_HIP_TRAINING_H

#include "iago_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * iago_value_mse_grad: the whole of train_value.py:53-57 -- pred = model(x), loss = mean_squared_error(pred, y),
 *   model.cleargrads(), loss.backward() -- for n rows of the Value net (network.py:66-96), in the split-f16 arithmetic
 *   of iago_policy_reinforce_grad (csrc/policy_grad_kernels.hip; the trunk, blocks 1..8, runs the same kernels):
 *   forward with every block's output kept, then the head and the loss forward and backward in float32:
 *     h9 = relu(conv3x3(x8; w9) + b9) [n][64],  h10 = w10 . h9,  d = h10 * (keep ? dropout_scale : 0),
 *     pred = w11 . d,  loss = sum (pred - y)^2 / n_mean,  dpred = float32(2 / n_mean) (pred - y),
 *   dw11, dh10 through the mask, dw10, dh9 masked by h9 > 0, dw9 / db9, and the gradient at block 8's
 *   pre-activations (masked by x8 > 0); from there blocks 8..2 and block 1 as iago_policy_reinforce_grad.
 *   Every sum has a fixed order (partial sums per workgroup, then a reduction launch): the same bits run after run.
 *   own / opp [n]: the positions, own = the side to move; result [n] float32 (y); keep: optional uint8 [n][128], the
 *   dropout mask of fc10's output (0 = dropped; NULL = no dropout, the eval-mode gradient); dropout_scale: the kept
 *   units' factor, float32(1 / (1 - 0.4)) as F.dropout scales (finite); n_mean: the row count the mean divides by.
 *   w1 [64][2][3][3], b1 [64]; blocks 2..8 as in iago_policy_grad_args; w9 [1][128][3][3], b9 [1], w10 [128][64],
 *   w11 [1][128].  g_*: the gradients in the parameters' own layouts; loss: device float; pred: optional [n], the
 *   model's output; h9: optional [n][64], block 9's output.  workspace: iago_value_grad_workspace_bytes(n) bytes,
 *   256-byte aligned.  overflow: bit 0 as for iago_conv3x3_split (the forward left the f16 range): that call's loss
 *   and gradients must not be used.  Returns IAGO_ERR_INVALID, before touching a device, on a NULL struct or
 *   pointer, n <= 0, n_mean <= 0, a workspace too small or misaligned, or a non-finite dropout_scale.
 */
typedef struct iago_value_grad_args {
    const uint64_t *own, *opp;
    const float *result;
    const uint8_t *keep;
    float dropout_scale;
    int64_t n, n_mean;
    const float *w1, *b1;
    const void *w_hi[7], *w_lo[7], *wt_hi[7], *wt_lo[7];
    const float *bias[7];
    const float *w9, *b9, *w10, *w11;
    float *g_w1, *g_b1;
    float *g_w[7], *g_b[7];
    float *g_w9, *g_b9, *g_w10, *g_w11;
    float *loss;
    float *pred, *h9;
    void *workspace;
    int64_t workspace_bytes;
    uint32_t *overflow;
} iago_value_grad_args;
/* bytes of the workspace of iago_value_mse_grad for n rows (-1 for n < 0) */
IAGO_API int64_t iago_value_grad_workspace_bytes(int64_t n);
IAGO_API int iago_value_mse_grad(const iago_value_grad_args *args, void *stream);

/*
 * iago_policy_visits_grad: SLPolicy trained on the search's own visit counts -- the cross-entropy of the model's
 *   output against the distribution of the root's visits (engine.SelfPlayResult.tuples()["pi"]) -- on the kernels of
 *   iago_policy_reinforce_grad (iago_hip.h): the same forward with every block's output kept, the same blocks 8..2,
 *   reduction and block 1; only the head and the loss differ.  Per row b, with n[a] = visits[b][a], N = sum_a n[a]
 *   (summed in integers) and w = weight[b]:
 *     logit = conv9 . x8 + bias10[cell],  m = max logit,  s = sum exp(logit - m),  p = exp(logit - m) / s
 *     t[a] = n[a] / N (float32),  row loss = w sum_{a: n[a] > 0} -t[a] ((logit[a] - m) - log s)
 *     loss = sum_b row loss / n_mean,  dlogits[a] = (w / n_mean) (p[a] - t[a])
 *   ONE softmax (the model's output), log p in its log-softmax form: a cell whose p underflowed keeps a finite log p.
 *   A row with N == 0 contributes nothing to the loss or to any gradient.  No temperature, no masking to the legal
 *   moves.  Deterministic (fixed summation orders), no host synchronisation.
 *   own / opp [n]: the searched positions, own = the mover; visits [n][64] int32, >= 0; weight: optional [n] float32
 *   (NULL = 1 for every row; rows added as padding carry 0 or all-zero visits); n_mean: the row count the mean divides
 *   by.  Weights, gradients, loss, probs and workspace (iago_policy_grad_workspace_bytes(n) bytes, 256-byte aligned)
 *   as in iago_policy_grad_args.  overflow: bit 0 as for iago_conv3x3_split (the forward left the f16 range); bit 1
 *   is raised by a negative count (that row contributes nothing): that call's loss and gradients must not be used.
 *   Returns IAGO_ERR_INVALID, before touching a device, on a NULL struct or required pointer, n <= 0, n_mean <= 0, or
 *   a workspace too small or misaligned.
 */
typedef struct iago_policy_visits_grad_args {
    const uint64_t *own, *opp;
    const int32_t *visits;
    const float *weight;
    int64_t n, n_mean;
    const float *w1, *b1;
    const void *w_hi[7], *w_lo[7], *wt_hi[7], *wt_lo[7];
    const float *bias[7];
    const float *w9, *b10;
    float *g_w1, *g_b1;
    float *g_w[7], *g_b[7];
    float *g_w9, *g_b10;
    float *loss;
    float *probs;
    void *workspace;
    int64_t workspace_bytes;
    uint32_t *overflow;
} iago_policy_visits_grad_args;
IAGO_API int iago_policy_visits_grad(const iago_policy_visits_grad_args *args, void *stream);

/*
 * iago_replay_sample: a minibatch out of a device-resident window of self-play rows, every row in one of the board's
 *   eight symmetries -- position, visit row and move together.  The window (all [capacity], slots 0 .. count-1
 *   filled): own / opp (own = the mover), pi [capacity][64] int32 (the root's visit counts by cell), move (int8, -1 =
 *   none), z (int8, the result from the mover's view).  1 <= count <= capacity < 2^31; n: the rows to produce.
 *   The draw of output row j (slot_in and sym_in both NULL), in integers, with replacement:
 *     c = Philox4x32-10 on the counter (uint32(j), step, 0, 0), key = seed with its high word XOR 0x52504C59 ("RPLY":
 *     key words seed & 0xFFFFFFFF and (seed >> 32) ^ 0x52504C59, as the explore draw of iago_mcts_search_explore
 *     splits its seed),  slot = (uint64(c[0]) * count) >> 32,  sym = c[1] & 7
 *   With slot_in (int32 [n]) and sym_in (uint8 [n]) both set the kernel takes them instead: the plain gather and
 *   transform (the full augmentation is this mode with sym = 0 .. 7 per row).  Exactly one of them: IAGO_ERR_INVALID.
 *   Variant k is iago_augment8's variant k (iago_hip.h): 0 the identity, 1 .. 3 successive counter-clockwise quarter
 *   turns (cell (y,x) -> (7-x, y)), 4 the transpose of variant 3, 5 .. 7 three more turns.  With m_k its cell map:
 *     own_out / opp_out have bit m_k(a) set where the source has bit a set,  pi_out[j][m_k(a)] = pi[slot][a],
 *     move_out = m_k(move) (-1 stays -1),  z_out = z,  result_out = float32(z) (optional: what iago_value_mse_grad
 *     takes),  slot_out / sym_out (optional): the row's slot and variant.
 *   A supplied slot outside [0, count) or sym > 7 is checked on the device: nothing is read for that row, it is
 *   written as zeros with move_out = -1 (slot_out / sym_out repeat what was supplied) and bit 0 of *flags (optional,
 *   one word, or-ed into: the caller clears it) is raised.  No floats in the draw, plain stores, no workspace.
 *   Returns IAGO_ERR_INVALID, before touching a device, on a NULL struct or required pointer, n <= 0, count <= 0,
 *   count > capacity, capacity >= 2^31, or only one of slot_in / sym_in.
 */
typedef struct iago_replay_sample_args {
    const uint64_t *own, *opp;
    const int32_t *pi;
    const int8_t *move, *z;
    int64_t capacity, count, n;
    uint64_t seed;
    uint32_t step, reserved0;
    const int32_t *slot_in;
    const uint8_t *sym_in;
    uint64_t *own_out, *opp_out;
    int32_t *pi_out;
    int8_t *move_out, *z_out;
    float *result_out;
    int32_t *slot_out;
    uint8_t *sym_out;
    uint32_t *flags;
} iago_replay_sample_args;
IAGO_API int iago_replay_sample(const iago_replay_sample_args *args, void *stream);

/*
 * iago_canonical_rows: the canonical form of n rows (own, opp), the one name all eight symmetries of a position share.
 *   With bb_k the board of variant k (iago_augment8's variants, in its order, as iago_replay_sample turns boards):
 *     k* = the lowest k in 0 .. 7 whose pair (bb_k(own), bb_k(opp)) is smallest -- own compared first, then opp, both
 *     as unsigned 64-bit;  c_own / c_opp [n] = that pair,  sym [n] (uint8) = k*.
 *   Rows are mover-relative (own = the mover), so colour plays no part.  Integers only, one thread per row.
 *   Returns IAGO_ERR_INVALID, before touching a device, on a NULL pointer or n <= 0.
 */
IAGO_API int iago_canonical_rows(const uint64_t *own, const uint64_t *opp, int64_t n, uint64_t *c_own, uint64_t *c_opp,
                                 uint8_t *sym, void *stream);

/*
 * iago_replay_merge: the filled slots 0 .. count-1 of a replay window merged by position up to symmetry.  A group is
 *   one distinct canonical pair (c_own, c_opp); groups are numbered in ascending (c_own, c_opp), compared as unsigned.
 *   The caller canonicalises (iago_canonical_rows over the window: c_own / c_opp / sym, by slot) and orders:
 *     order [count] int32: the slots in ascending (c_own, c_opp) (ties in any order: integer sums do not depend on it),
 *     group [count] int32: the group number of order[i] -- 0 at i = 0, then the predecessor's or one more.
 *   Group g then holds, all [count]-sized buffers of which the first n_unique entries are written:
 *     own_out[g] / opp_out[g]  the canonical boards,
 *     pi_out[g][d] (int32)     the sum over its rows of pi[slot][a] with m_sym[slot](a) = d: the visit row turned into
 *                              the canonical frame exactly as iago_replay_sample turns it by variant sym[slot],
 *     z_sum[g] (int32)         the sum of z,   mult[g] (int32) the number of its rows,
 *     first[g] (int64)         the exclusive prefix sum of mult (the group's first sorted row),
 *     *n_unique (int32)        the number of groups.
 *   Sums are accumulated in 64 bits; a cell or z_sum that would leave int32 is stored as the nearest end of its range
 *   (2^31 - 1 above) and raises IAGO_REPLAY_MERGE_OVERFLOW in *flags.  The device checks what it indexes by: a group
 *   numbering that breaks the rule above merges nothing (*n_unique = 0), a row whose slot lies outside [0, count),
 *   whose sym is above 7 or whose canonical boards differ from those of its group's first row is left out; each raises
 *   IAGO_REPLAY_MERGE_BAD_INPUT.  flags: one word, or-ed into; the caller clears it before the call.
 *   One wave per group, lane = canonical cell, plain stores.  A group of more than 512 rows (the start position, once
 *   per game of the window) is first summed by one wave per 256 sorted rows, which add their parts with 64-bit integer
 *   atomics into workspace ([count] int64, need not be initialised: the call clears it); integer sums, so the result
 *   is the same bits whatever the schedule.  No waiting on the device.
 *   Returns IAGO_ERR_INVALID, before touching a device, on a NULL struct or pointer, count <= 0 or count >= 2^31.
 */
#define IAGO_REPLAY_MERGE_BAD_INPUT 1
#define IAGO_REPLAY_MERGE_OVERFLOW 2
typedef struct iago_replay_merge_args {
    const uint64_t *c_own, *c_opp;
    const uint8_t *sym;
    const int32_t *pi;
    const int8_t *z;
    int64_t count;
    const int32_t *order, *group;
    uint64_t *own_out, *opp_out;
    int32_t *pi_out, *z_sum, *mult;
    int64_t *first;
    int64_t *workspace;
    int32_t *n_unique;
    uint32_t *flags;
} iago_replay_merge_args;
IAGO_API int iago_replay_merge(const iago_replay_merge_args *args, void *stream);

/*
 * iago_replay_sample_merged: a minibatch out of the merged rows of iago_replay_merge (own / opp / pi / z_sum / mult /
 *   first, n_unique groups of a window of count rows), every row in one of the board's eight symmetries.  The draw of
 *   output row j is iago_replay_sample's: c = Philox4x32-10 on the counter (uint32(j), step, 0, 0) under the same key
 *   split of seed,  sym = c[1] & 7,  and the group g by mode:
 *     IAGO_REPLAY_MERGED_UNIQUE  g = (uint64(c[0]) * n_unique) >> 32: uniform over positions;
 *     IAGO_REPLAY_MERGED_ROWS    r = (uint64(c[0]) * count) >> 32, g the group with first[g] <= r < first[g] + mult[g]
 *                                (binary search on first): positions keep the weight they have in the window.
 *   Outputs [n]: own_out / opp_out = variant sym of the canonical boards,  pi_out[j][m_sym(a)] = pi[g][a] (int32),
 *   result_out = float32(z_sum[g]) / float32(mult[g]) (one conversion each, one IEEE division),  z_sum_out, mult_out,
 *   group_out (int32), sym_out (uint8).  No move or z columns: a merged row has neither.  Integers but for that
 *   division, plain stores, no workspace.
 *   Returns IAGO_ERR_INVALID, before touching a device, on a NULL struct or pointer, n <= 0, n_unique <= 0,
 *   n_unique > count, count >= 2^31, or another mode.
 */
#define IAGO_REPLAY_MERGED_UNIQUE 0
#define IAGO_REPLAY_MERGED_ROWS 1
typedef struct iago_replay_sample_merged_args {
    const uint64_t *own, *opp;
    const int32_t *pi, *z_sum, *mult;
    const int64_t *first;
    int64_t n_unique, count, n;
    uint64_t seed;
    uint32_t step;
    int32_t mode;
    uint64_t *own_out, *opp_out;
    int32_t *pi_out;
    float *result_out;
    int32_t *z_sum_out, *mult_out, *group_out;
    uint8_t *sym_out;
} iago_replay_sample_merged_args;
IAGO_API int iago_replay_sample_merged(const iago_replay_sample_merged_args *args, void *stream);

/*
 * iago_value_targets: the Value net's targets of a round of recorded games from the search's own values -- the game's
 *   result z mixed with the roots' values (iago_mcts_root_value, iago_hip_serving.h) and TD(lambda) returns along the
 *   game, in 64-bit integers, Q16.  The records are SelfPlayResult's, [n_turns][n_games], turn-major:
 *     valid (uint8)  1 / 4: the turn was searched (a full / a fast turn), 3: the endgame solver played it; 0, 2 and 5 (a
 *                    pass or no turn, a move without a search, a random opening move) are NO rows,
 *     q (int32)      the root's value from the MOVER's view in Q16 on the searched rows,
 *     score (int8)   the exact final disc difference from the mover's view on the solved rows,
 *     z (int8) [n_games] the game's result from colour 1's view,   mover (int8) [n_turns] the colour to move (1 or 2).
 *   The rule, in colour 1's frame.  s_t = +1 where mover[t] == 1, else -1;  Z = 65536 z[b];
 *     V_t = s_t clip(q[t][b], -65536, 65536) on a searched row,  V_t = s_t 65536 sign(score[t][b]) on a solved row.
 *   Start with Gnext = Vnext = Z.  For t = n_turns - 1 .. 0, on a row:
 *     G_t = ((256 - lam_256) Vnext + lam_256 Gnext + 128) >> 8     (an arithmetic shift: it floors),
 *     R_t = ((256 - mix_256) G_t + mix_256 V_t + 128) >> 8,
 *     out[t][b] = s_t R_t (int32: the target from the MOVER's view, |out| <= 65536),  then Gnext = G_t, Vnext = V_t.
 *   Where there is no row out[t][b] = 0 and the chain stays as it is.  G is the TD(lambda) return of the position AFTER
 *   which it stands, lambda = lam_256 / 256, without the row's own value; mix_256 / 256 of the row's own value joins it.
 *   (256, 0): exactly 65536 z from the mover's view, the label of before.  (256, 128): the z-q average.  (0, 0): one-step
 *   bootstrapping -- every row takes the next row's V, the last one Z.
 *   One lane per game walking backward over the turns (a wave's loads of a record row are contiguous), no LDS, no
 *   scratch memory, plain stores.
 *   Returns IAGO_ERR_INVALID, before touching a device, on a NULL struct or pointer, n_turns <= 0, n_games <= 0,
 *   n_turns * n_games > 2^31, lam_256 or mix_256 outside [0, 256].
 */
typedef struct iago_value_targets_args {
    const uint8_t *valid;
    const int32_t *q;
    const int8_t *score, *z, *mover;
    int64_t n_turns, n_games;
    int32_t lam_256, mix_256;
    int32_t *out;
} iago_value_targets_args;
IAGO_API int iago_value_targets(const iago_value_targets_args *args, void *stream);

/*
 * iago_replay_merge_values: an int32 column of the window (v, by slot: the value targets) summed per group of a merge --
 *   order / group [count] as iago_replay_merge took them, first (int64) / mult (int32) [n_unique] as it wrote them:
 *     v_sum[g] (int64) = the sum of v[order[i]] over first[g] <= i < first[g] + mult[g].
 *   A value is invariant under the board's symmetries: no variant enters.  One wave per group, the lanes striding over
 *   the group's sorted rows, a 64-bit wave reduction, plain stores and no atomics on the sums: the bits do not depend on
 *   the schedule.  The device checks what it indexes by: a span outside the sorted order is clamped into it, a row whose
 *   slot lies outside [0, count) or whose group[i] is not g is left out; each raises IAGO_REPLAY_MERGE_BAD_INPUT in
 *   *flags (optional, one word, or-ed into; the caller clears it).
 *   Returns IAGO_ERR_INVALID, before touching a device, on a NULL struct or pointer (flags aside), count <= 0,
 *   count >= 2^31, n_unique <= 0 or n_unique > count.
 */
typedef struct iago_replay_merge_values_args {
    const int32_t *order, *group;
    const int64_t *first;
    const int32_t *mult, *v;
    int64_t count, n_unique;
    int64_t *v_sum;
    uint32_t *flags;
} iago_replay_merge_values_args;
IAGO_API int iago_replay_merge_values(const iago_replay_merge_values_args *args, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* IAGO_HIP_TRAINING_H */
