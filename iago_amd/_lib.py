"""ctypes binding of the C ABI declared in include/iago_hip.h.

There is no CPU fallback.  If libiago_hip.so has not been built, importing
anything that needs it raises; if it is loaded on a host without a HIP device,
every launch returns IAGO_ERR_HIP and `check` raises.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("IAGO_HIP_LIB") or os.path.join(HERE, "libiago_hip.so")

IAGO_OK = 0
IAGO_ERR_INVALID, IAGO_ERR_HIP, IAGO_ERR_CAPACITY = -1, -2, -3
IAGO_MAX_TURNS = 128
IAGO_ROLLOUT_TABLE_FLOATS = 3 * 2 * 256 * 8 + 64 + 4 + 2 * 512
ROLLOUT_MODE_INDEX = 3 * 2 * 256 * 8 + 64  # blob[mode] == 1.0: product form
TRACE_PASS = 0xFF

# every symbol include/iago_hip.h declares -- the drop-in boundary: what a binding of the reference's hot path calls
# (tests/test_abi.py checks the lists against the headers and the built library)
SYMBOLS = [
    "iago_abi_version", "iago_last_error", "iago_device_count",
    "iago_legal_moves", "iago_apply_moves", "iago_play_turn", "iago_encode_planes", "iago_encode_planes_indexed",
    "iago_judge", "iago_sample_moves", "iago_augment8",
    "iago_rollout_build_table", "iago_rollout",
    "iago_policy_forward_split3", "iago_value_forward_split", "iago_value_rollout",
    "iago_mcts_reset", "iago_leaf_values", "iago_mcts_best_move", "iago_mcts_advance_root", "iago_mcts_compact",
    "iago_mcts_mix_backup_lookahead", "iago_mcts_store_priors", "iago_mcts_descend",
    "iago_mcts_search_persistent", "iago_mcts_search_capacity", "iago_mcts_search_streams_create",
    "iago_mcts_search_streams_destroy", "iago_mcts_search_split", "iago_selfplay_policy",
    "iago_policy_grad_workspace_bytes", "iago_policy_reinforce_grad", "iago_adam_chainer",
]
# include/iago_hip_layers.h: single blocks, the ends of the nets, format conversions, a block's three gradient kernels
# (the modules' planes-fed forwards of small batches, the layer-by-layer cross-checks of the fused kernels)
LAYER_SYMBOLS = [
    "iago_bias_relu", "iago_conv3x3_split", "iago_conv3x3_split_trunk", "iago_split_nchw", "iago_merge_nchw",
    "iago_value_stem", "iago_value_stem_boards", "iago_value_head",
    "iago_conv3x3_f32", "iago_stem_f32", "iago_stem_f32_boards", "iago_policy_head",
    "iago_conv3x3_wgrad_split", "iago_conv3x3_bwd_data_split", "iago_split_scaled",
]
# include/iago_hip_experimental.h, outside the boundary: two schedules of the per-playout engine that measured slower
# (game-asynchronous steps, value look-ahead: engine.BatchedMCTS(async_steps=True / value_ahead=True)); the per-phase forms
# of a playout (arbitrary callables as nets, the IAGO_FUSED_* = 0 knobs)
EXPERIMENTAL_SYMBOLS = [
    "iago_value_rollout_async", "iago_value_forward_batch", "iago_mcts_value_ahead_rows", "iago_mcts_value_ahead_store",
    "iago_mcts_select", "iago_mcts_expand", "iago_mcts_pending", "iago_mcts_backup", "iago_mcts_mix_backup",
    "iago_mcts_expand_cached", "iago_mcts_fresh_leaves",
]
# include/iago_hip_serving.h: searching ONE position fast -- W playouts of a tree in flight (engine.BatchedMCTS(wave=W)),
# the exact endgame solver (ops.solve_endgame, engine.solve_endgame; every optimal move and every move's value:
# ops.solve_endgame_moves, engine.endgame_errors, SelfPlayEngine.play(solved_targets=True)), exploring self-play (SelfPlayEngine.play(explore_turns=)),
# playout-cap randomisation (SelfPlayEngine.play(playout_cap=)), root noise (SelfPlayEngine.play(root_noise=)), forced
# playouts and policy-target pruning (SelfPlayEngine.play(forced_playouts=)), the fixed-depth alpha-beta opponent and its
# random openings (ops.alphabeta_moves, ops.random_moves; SelfPlayEngine.play_match(opponent=AlphaBeta(d))), that
# search with every root spread over the lanes (ops.alphabeta_moves(split=), AlphaBeta(d, split)), and the exact solver
# spread the same way (ops.solve_endgame(split=), ops.solve_endgame_moves(split=)), and the Gumbel root search
# (SelfPlayEngine.play(gumbel=), BatchedMCTS.search(gumbel=)), and the root's value read back after a search
# (ops.mcts_root_value, BatchedMCTS.root_value, SelfPlayEngine.play(root_values=True))
SERVING_SYMBOLS = [
    "iago_mcts_search_wave", "iago_solve_endgame", "iago_play_endgame", "iago_mcts_search_park",
    "iago_solve_endgame_moves", "iago_play_endgame_moves",
    "iago_mcts_search_explore", "iago_mcts_draw_move", "iago_mcts_search_arena",
    "iago_mcts_search_cap", "iago_mcts_cap_mask",
    "iago_mcts_root_noise", "iago_mcts_search_noise",
    "iago_mcts_search_forced", "iago_mcts_prune_visits", "iago_mcts_prune_visits_rule",
    "iago_alphabeta_moves", "iago_random_moves", "iago_alphabeta_moves_split", "iago_solve_endgame_split",
    "iago_mcts_gumbel_draw", "iago_mcts_search_gumbel", "iago_mcts_gumbel_finish",
    "iago_mcts_root_value",
]
# include/iago_hip_training.h: training the nets on the library's kernels -- the Value net's supervised update
# (network.Value.value_grads, train_supervised.SupervisedTrainer(native=True)), SLPolicy on the search's visit counts
# (network.SLPolicy.visits_grads, train_rl.ReinforceTrainer.step_from_tuples(target="visits")), minibatches out of a
# replay window of self-play rows in random board symmetries (ops.replay_sample, replay.ReplayWindow), the rows'
# canonical forms, the window merged by position up to symmetry and minibatches out of the merged rows
# (ops.canonical_rows, ops.replay_merge, ops.replay_sample_merged, ReplayWindow.merge / sample(merged=)), the Value
# net's targets from the search's root values -- z mixed with q, TD(lambda) along the game -- and their sums per merged
# position (ops.value_targets, SelfPlayResult.value_targets, ops.replay_merge_values, ReplayWindow(value_targets=True))
TRAINING_SYMBOLS = [
    "iago_value_grad_workspace_bytes", "iago_value_mse_grad", "iago_policy_visits_grad", "iago_replay_sample",
    "iago_canonical_rows", "iago_replay_merge", "iago_replay_sample_merged",
    "iago_value_targets", "iago_replay_merge_values",
]


class IagoError(RuntimeError):
    pass


class RolloutArgs(C.Structure):
    _fields_ = [
        ("own", C.c_void_p), ("opp", C.c_void_p), ("n", C.c_int64),
        ("table", C.c_void_p), ("uniforms", C.c_void_p),
        ("seed", C.c_uint64), ("id_base", C.c_uint32), ("stream_id", C.c_uint32),
        ("stream_id_dev", C.c_void_p),
        ("z", C.c_void_p), ("final_own", C.c_void_p), ("final_opp", C.c_void_p),
        ("n_turns", C.c_void_p), ("trace", C.c_void_p), ("log_form", C.c_int),
        ("throughput_hint", C.c_int),
    ]


ADAM_MAX_TENSORS = 24


class AdamArgs(C.Structure):
    _fields_ = [
        ("p", C.c_void_p * ADAM_MAX_TENSORS), ("g", C.c_void_p * ADAM_MAX_TENSORS),
        ("m", C.c_void_p * ADAM_MAX_TENSORS), ("v", C.c_void_p * ADAM_MAX_TENSORS),
        ("step", C.c_void_p * ADAM_MAX_TENSORS),
        ("count", C.c_int64 * ADAM_MAX_TENSORS), ("n_tensors", C.c_int32),
        ("alpha_t", C.c_float), ("one_minus_beta1", C.c_float), ("one_minus_beta2", C.c_float),
        ("eps", C.c_float), ("weight_decay", C.c_float),
    ]


class PolicyGradArgs(C.Structure):
    _fields_ = [
        ("own", C.c_void_p), ("opp", C.c_void_p), ("action", C.c_void_p), ("reward", C.c_void_p),
        ("n", C.c_int64), ("n_mean", C.c_int64),
        ("w1", C.c_void_p), ("b1", C.c_void_p),
        ("w_hi", C.c_void_p * 7), ("w_lo", C.c_void_p * 7), ("wt_hi", C.c_void_p * 7), ("wt_lo", C.c_void_p * 7),
        ("bias", C.c_void_p * 7),
        ("w9", C.c_void_p), ("b10", C.c_void_p),
        ("g_w1", C.c_void_p), ("g_b1", C.c_void_p),
        ("g_w", C.c_void_p * 7), ("g_b", C.c_void_p * 7),
        ("g_w9", C.c_void_p), ("g_b10", C.c_void_p),
        ("loss", C.c_void_p), ("probs", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
        ("overflow", C.c_void_p),
    ]


class PolicyVisitsGradArgs(C.Structure):
    """Mirror of iago_policy_visits_grad_args (include/iago_hip_training.h): PolicyGradArgs with action / reward
    replaced by visits / weight."""
    _fields_ = [("visits", t) if f == "action" else ("weight", t) if f == "reward" else (f, t)
                for f, t in PolicyGradArgs._fields_]


class ValueGradArgs(C.Structure):
    """Mirror of iago_value_grad_args (include/iago_hip_training.h)."""
    _fields_ = [
        ("own", C.c_void_p), ("opp", C.c_void_p), ("result", C.c_void_p), ("keep", C.c_void_p),
        ("dropout_scale", C.c_float),
        ("n", C.c_int64), ("n_mean", C.c_int64),
        ("w1", C.c_void_p), ("b1", C.c_void_p),
        ("w_hi", C.c_void_p * 7), ("w_lo", C.c_void_p * 7), ("wt_hi", C.c_void_p * 7), ("wt_lo", C.c_void_p * 7),
        ("bias", C.c_void_p * 7),
        ("w9", C.c_void_p), ("b9", C.c_void_p), ("w10", C.c_void_p), ("w11", C.c_void_p),
        ("g_w1", C.c_void_p), ("g_b1", C.c_void_p),
        ("g_w", C.c_void_p * 7), ("g_b", C.c_void_p * 7),
        ("g_w9", C.c_void_p), ("g_b9", C.c_void_p), ("g_w10", C.c_void_p), ("g_w11", C.c_void_p),
        ("loss", C.c_void_p), ("pred", C.c_void_p), ("h9", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
        ("overflow", C.c_void_p),
    ]


REPLAY_KEY = 0x52504C59   # a replay window's draws: Philox key = the window's seed with its high word XOR this ("RPLY")
REPLAY_BAD_ROW = 1        # bit of iago_replay_sample's flags: a supplied slot or variant was out of range


class ReplaySampleArgs(C.Structure):
    """Mirror of iago_replay_sample_args (include/iago_hip_training.h)."""
    _fields_ = [
        ("own", C.c_void_p), ("opp", C.c_void_p), ("pi", C.c_void_p), ("move", C.c_void_p), ("z", C.c_void_p),
        ("capacity", C.c_int64), ("count", C.c_int64), ("n", C.c_int64),
        ("seed", C.c_uint64), ("step", C.c_uint32), ("reserved0", C.c_uint32),
        ("slot_in", C.c_void_p), ("sym_in", C.c_void_p),
        ("own_out", C.c_void_p), ("opp_out", C.c_void_p), ("pi_out", C.c_void_p), ("move_out", C.c_void_p),
        ("z_out", C.c_void_p), ("result_out", C.c_void_p), ("slot_out", C.c_void_p), ("sym_out", C.c_void_p),
        ("flags", C.c_void_p),
    ]


REPLAY_MERGE_BAD_INPUT = 1   # bits of iago_replay_merge's flags: an order / group / slot the device refused,
REPLAY_MERGE_OVERFLOW = 2    # a summed cell or z_sum left int32 (stored clamped)
REPLAY_MERGED_MODES = {"unique": 0, "rows": 1}   # iago_replay_sample_merged's mode


class ReplayMergeArgs(C.Structure):
    """Mirror of iago_replay_merge_args (include/iago_hip_training.h)."""
    _fields_ = [
        ("c_own", C.c_void_p), ("c_opp", C.c_void_p), ("sym", C.c_void_p), ("pi", C.c_void_p), ("z", C.c_void_p),
        ("count", C.c_int64), ("order", C.c_void_p), ("group", C.c_void_p),
        ("own_out", C.c_void_p), ("opp_out", C.c_void_p), ("pi_out", C.c_void_p), ("z_sum", C.c_void_p),
        ("mult", C.c_void_p), ("first", C.c_void_p), ("workspace", C.c_void_p), ("n_unique", C.c_void_p),
        ("flags", C.c_void_p),
    ]


class ReplaySampleMergedArgs(C.Structure):
    """Mirror of iago_replay_sample_merged_args (include/iago_hip_training.h)."""
    _fields_ = [
        ("own", C.c_void_p), ("opp", C.c_void_p), ("pi", C.c_void_p), ("z_sum", C.c_void_p), ("mult", C.c_void_p),
        ("first", C.c_void_p),
        ("n_unique", C.c_int64), ("count", C.c_int64), ("n", C.c_int64),
        ("seed", C.c_uint64), ("step", C.c_uint32), ("mode", C.c_int32),
        ("own_out", C.c_void_p), ("opp_out", C.c_void_p), ("pi_out", C.c_void_p), ("result_out", C.c_void_p),
        ("z_sum_out", C.c_void_p), ("mult_out", C.c_void_p), ("group_out", C.c_void_p), ("sym_out", C.c_void_p),
    ]


class ValueTargetsArgs(C.Structure):
    """Mirror of iago_value_targets_args (include/iago_hip_training.h)."""
    _fields_ = [
        ("valid", C.c_void_p), ("q", C.c_void_p), ("score", C.c_void_p), ("z", C.c_void_p), ("mover", C.c_void_p),
        ("n_turns", C.c_int64), ("n_games", C.c_int64), ("lam_256", C.c_int32), ("mix_256", C.c_int32),
        ("out", C.c_void_p),
    ]


class ReplayMergeValuesArgs(C.Structure):
    """Mirror of iago_replay_merge_values_args (include/iago_hip_training.h)."""
    _fields_ = [
        ("order", C.c_void_p), ("group", C.c_void_p), ("first", C.c_void_p), ("mult", C.c_void_p), ("v", C.c_void_p),
        ("count", C.c_int64), ("n_unique", C.c_int64), ("v_sum", C.c_void_p), ("flags", C.c_void_p),
    ]


VALUE_Q16 = 65536             # a value target, a root value: Q16 (iago_value_targets, iago_mcts_root_value)
ROOT_VALUE_SATURATED = 1      # IAGO_ROOT_VALUE_SATURATED: bits of iago_mcts_root_value's flags
ROOT_VALUE_NAN = 2            # IAGO_ROOT_VALUE_NAN


class ConvSplitLayer(C.Structure):
    """Mirror of iago_conv_split_layer (include/iago_hip.h)."""
    _fields_ = [
        ("x_hi", C.c_void_p), ("x_lo", C.c_void_p), ("w_hi", C.c_void_p), ("w_lo", C.c_void_p),
        ("bias", C.c_void_p), ("y_hi", C.c_void_p), ("y_lo", C.c_void_p),
        ("cin", C.c_int32), ("reserved", C.c_int32),
    ]


class PolicySplit3Args(C.Structure):
    """Mirror of iago_policy_split3_args (include/iago_hip.h)."""
    _fields_ = [
        ("own", C.c_void_p), ("opp", C.c_void_p), ("index", C.c_void_p), ("n_dev", C.c_void_p), ("n", C.c_int64),
        ("w1", C.c_void_p), ("b1", C.c_void_p),
        ("w_hi", C.c_void_p * 7), ("w_mid", C.c_void_p * 7), ("w_lo", C.c_void_p * 7), ("bias", C.c_void_p * 7),
        ("w9", C.c_void_p), ("b10", C.c_void_p), ("probs", C.c_void_p), ("overflow", C.c_void_p),
        ("parts", C.c_int32), ("scratch_rows", C.c_int32), ("scratch", C.c_void_p),
    ]


class SelfplayPolicyArgs(C.Structure):
    """Mirror of iago_selfplay_policy_args (include/iago_hip.h)."""
    _fields_ = [
        ("model1", C.c_void_p), ("model2", C.c_void_p), ("own", C.c_void_p), ("opp", C.c_void_p), ("n", C.c_int64),
        ("seed", C.c_uint64), ("id_base", C.c_uint32), ("max_turns", C.c_int32),
        ("rec_own", C.c_void_p), ("rec_opp", C.c_void_p), ("rec_act", C.c_void_p), ("n_turns", C.c_void_p),
        ("bad_probs", C.c_void_p),
    ]


class MctsAsync(C.Structure):
    """Mirror of iago_mcts_async (include/iago_hip.h)."""
    _fields_ = [
        ("parts", C.c_int32), ("reserved", C.c_int32), ("wait", C.c_void_p), ("done", C.c_void_p),
        ("roll", C.c_void_p), ("fq_index", C.c_void_p), ("fq_count", C.c_void_p), ("step", C.c_void_p),
        ("n_sims", C.c_void_p), ("scratch", C.c_void_p),
    ]


VALUE_IMAGE_BYTES = 34816   # IAGO_VALUE_IMAGE_BYTES


class MctsLookahead(C.Structure):
    """Mirror of iago_mcts_lookahead (include/iago_hip.h)."""
    _fields_ = [
        ("trigger", C.c_int32), ("slots", C.c_int32), ("next_seq", C.c_void_p), ("cache_seq", C.c_void_p),
        ("cache", C.c_void_p), ("q_count", C.c_void_p), ("q_capacity", C.c_int32), ("path_stride", C.c_int32),
        ("q_own", C.c_void_p), ("q_opp", C.c_void_p), ("q_game", C.c_void_p), ("q_seq", C.c_void_p),
        ("error", C.c_void_p), ("clear_word", C.c_void_p), ("path", C.c_void_p), ("path_len", C.c_void_p),
        ("z_log", C.c_void_p), ("z_log_n", C.c_void_p), ("z_log_rows", C.c_int32), ("reserved", C.c_int32),
        ("async_", C.c_void_p), ("value_ahead", C.c_void_p),
    ]


class MctsValueAhead(C.Structure):
    """Mirror of iago_mcts_value_ahead (include/iago_hip.h)."""
    _fields_ = [
        ("x_capacity", C.c_int32), ("row_capacity", C.c_int32), ("x_count", C.c_void_p),
        ("x_game", C.c_void_p), ("x_node", C.c_void_p), ("x_own", C.c_void_p), ("x_opp", C.c_void_p),
        ("row_count", C.c_void_p), ("row_own", C.c_void_p), ("row_opp", C.c_void_p), ("row_node", C.c_void_p),
        ("row_v", C.c_void_p), ("total", C.c_void_p),
    ]


SEARCH_QUEUE_ENTRIES = 4096   # IAGO_SEARCH_QUEUE_ENTRIES
SEARCH_GAMES_PER_WORKGROUP = 32   # IAGO_SEARCH_GAMES_PER_WORKGROUP
SEARCH_CHAIN_SKIP = 0x100         # IAGO_SEARCH_CHAIN_SKIP (OR-ed into games_per_workgroup; totals is then [17])
SEARCH_NEGAMAX = 0x200            # IAGO_SEARCH_NEGAMAX (include/iago_hip_serving.h; OR-ed in likewise: the negamax backup rule)
SEARCH_PUCT_AZ = 0x400            # IAGO_SEARCH_PUCT_AZ (include/iago_hip_serving.h; OR-ed in likewise: the AlphaZero selection rule)
# whole-game launches (max_turns > 0, games_total = 0): iago_mcts_search_args.active[g] selects the game's kind
MATCH_MCTS_COLOUR_1 = 2   # a match: PV-MCTS plays colour 1 (moves first), the SL policy colour 2
MATCH_MCTS_COLOUR_2 = 3   # a match: PV-MCTS plays colour 2, the SL policy colour 1 (the reference's game.py --auto)
MATCH_KEY = 0x4D415443    # a match's policy draws: Philox key = the rollout seed with its high word XOR this
MATCH_SEED_XOR = MATCH_KEY << 32
EXPLORE_KEY = 0x4558504C  # exploring self-play's draws from the visit counts: the same, with this word (IAGO_EXPLORE_KEY)
EXPLORE_SEED_XOR = EXPLORE_KEY << 32
CAP_KEY = 0x43415050      # the playout cap's full / fast decision per turn: the same, with this word (IAGO_CAP_KEY)
CAP_SEED_XOR = CAP_KEY << 32
NOISE_KEY = 0x44495249    # the root noise's urn draws: the same, with this word (IAGO_NOISE_KEY)
NOISE_SEED_XOR = NOISE_KEY << 32
GUMBEL_KEY = 0x47554D42   # the Gumbel root search's draws: the same, with this word (IAGO_GUMBEL_KEY)
GUMBEL_SEED_XOR = GUMBEL_KEY << 32
GUMBEL_C_VISIT = 50       # gumbel=(m, c_scale_256): sigma's c_visit unless the caller gives a third number
NOISE_DRAWS = 256         # root_noise=(alpha_256, eps_256): the urn's draws N unless the caller gives a third number
CTL_BAD_DRAW = 13         # ctl word a match raises when a policy draw found no mass on the legal moves
REC_DRAWN = 2             # rec_valid of a move played without a search (a policy draw or a forced final move)
REC_FAST = 4              # rec_valid of a searched FAST turn of the playout cap (n_fast playouts; not a policy target)
REC_OPENING = 5           # rec_valid of a random opening move (play_match(opening_turns=): nobody searched)
OPENING_KEY = 0x4F50454E  # a match's random openings: Philox key = the seed with its high word XOR this (IAGO_OPENING_KEY)
OPENING_SEED_XOR = OPENING_KEY << 32


class MctsSearchArgs(C.Structure):
    """Mirror of iago_mcts_search_args (include/iago_hip.h)."""
    _fields_ = [
        ("tree", C.c_void_p), ("root_own", C.c_void_p), ("root_opp", C.c_void_p), ("active", C.c_void_p),
        ("c_puct", C.c_float), ("lmbda", C.c_float), ("n_thr", C.c_int32), ("n_sims", C.c_int32),
        ("net_workgroups", C.c_int32), ("time_limit_ms", C.c_int32),
        ("value", C.c_void_p), ("policy", C.c_void_p), ("rollout", C.c_void_p),
        ("cur_node", C.c_void_p), ("cur_own", C.c_void_p), ("cur_opp", C.c_void_p), ("path", C.c_void_p),
        ("path_stride", C.c_int32), ("z_log_rows", C.c_int32), ("done", C.c_void_p), ("roll", C.c_void_p),
        ("leaf_value", C.c_void_p), ("z_log", C.c_void_p), ("z_log_n", C.c_void_p), ("q_slots", C.c_void_p),
        ("ctl", C.c_void_p), ("rep_v", C.c_void_p), ("rep_p", C.c_void_p), ("totals", C.c_void_p),
        ("stats", C.c_void_p), ("wg_own", C.c_void_p), ("wg_opp", C.c_void_p),
        ("max_turns", C.c_int32), ("games_per_workgroup", C.c_int32), ("game_own", C.c_void_p), ("game_opp", C.c_void_p),
        ("n_turns", C.c_void_p), ("rec_own", C.c_void_p), ("rec_opp", C.c_void_p), ("rec_valid", C.c_void_p),
        ("rec_move", C.c_void_p), ("rec_pi", C.c_void_p),
        ("vtable", C.c_void_p), ("vtable_slots", C.c_int64),
        ("trace", C.c_void_p), ("trace_rows", C.c_int32), ("pace_margin", C.c_int32),
        ("max_cus", C.c_int32), ("games_total", C.c_int32),
    ]


class SearchWaveArgs(C.Structure):
    """Mirror of iago_search_wave_args (include/iago_hip_serving.h)."""
    _fields_ = [
        ("width", C.c_int32), ("vloss", C.c_float), ("timing", C.c_void_p), ("reserved", C.c_int64 * 4),
    ]


ENDGAME_EXACT = 0          # IAGO_ENDGAME_EXACT
ENDGAME_WLD = 1            # IAGO_ENDGAME_WLD
ENDGAME_MAX_EMPTIES = 20   # IAGO_ENDGAME_MAX_EMPTIES
ENDGAME_MAX_TIME_MS = 600000
ENDGAME_CTL_WORDS = 4


class EndgameArgs(C.Structure):
    """Mirror of iago_endgame_args (include/iago_hip_serving.h)."""
    _fields_ = [
        ("own", C.c_void_p), ("opp", C.c_void_p), ("n", C.c_int64),
        ("mode", C.c_int32), ("max_empties", C.c_int32), ("time_limit_ms", C.c_int32), ("reserved0", C.c_int32),
        ("score", C.c_void_p), ("move", C.c_void_p), ("nodes", C.c_void_p), ("solved", C.c_void_p),
        ("ctl", C.c_void_p), ("reserved", C.c_int64 * 4),
    ]


class PlayEndgameArgs(C.Structure):
    """Mirror of iago_play_endgame_args (include/iago_hip_serving.h)."""
    _fields_ = [
        ("own", C.c_void_p), ("opp", C.c_void_p), ("turn", C.c_void_p), ("stones", C.c_void_p),
        ("pass_flg", C.c_void_p), ("parked", C.c_void_p), ("n", C.c_int64), ("stride", C.c_int64),
        ("max_turns", C.c_int32), ("max_empties", C.c_int32), ("time_limit_ms", C.c_int32), ("reserved0", C.c_int32),
        ("rec_own", C.c_void_p), ("rec_opp", C.c_void_p), ("rec_valid", C.c_void_p), ("rec_move", C.c_void_p),
        ("rec_score", C.c_void_p), ("finished", C.c_void_p), ("ctl", C.c_void_p), ("reserved", C.c_int64 * 4),
    ]


ENDGAME_MOVES_BEST = 0     # IAGO_ENDGAME_MOVES_BEST
ENDGAME_MOVES_ALL = 1      # IAGO_ENDGAME_MOVES_ALL
ENDGAME_NO_MOVE = -128     # IAGO_ENDGAME_NO_MOVE


class EndgameMovesArgs(C.Structure):
    """Mirror of iago_endgame_moves_args (include/iago_hip_serving.h)."""
    _fields_ = [
        ("own", C.c_void_p), ("opp", C.c_void_p), ("n", C.c_int64),
        ("mode", C.c_int32), ("moves", C.c_int32), ("max_empties", C.c_int32), ("time_limit_ms", C.c_int32),
        ("score", C.c_void_p), ("move", C.c_void_p), ("nodes", C.c_void_p), ("solved", C.c_void_p),
        ("best", C.c_void_p), ("move_score", C.c_void_p), ("ctl", C.c_void_p), ("reserved", C.c_int64 * 4),
    ]


ENDGAME_MAX_SPLIT = 2         # IAGO_ENDGAME_MAX_SPLIT
ENDGAME_SPLIT_CTL_WORDS = 8   # IAGO_ENDGAME_SPLIT_CTL_WORDS


class EndgameSplitArgs(C.Structure):
    """Mirror of iago_endgame_split_args (include/iago_hip_serving.h)."""
    _fields_ = [
        ("own", C.c_void_p), ("opp", C.c_void_p), ("n", C.c_int64),
        ("mode", C.c_int32), ("split", C.c_int32), ("max_empties", C.c_int32), ("time_limit_ms", C.c_int32),
        ("score", C.c_void_p), ("move", C.c_void_p), ("nodes", C.c_void_p), ("solved", C.c_void_p),
        ("best", C.c_void_p), ("move_score", C.c_void_p),
        ("job_count", C.c_void_p), ("job_first", C.c_void_p), ("job_capacity", C.c_int64),
        ("job_own", C.c_void_p), ("job_opp", C.c_void_p), ("job_root", C.c_void_p), ("job_path", C.c_void_p),
        ("job_score", C.c_void_p), ("job_move", C.c_void_p), ("job_nodes", C.c_void_p), ("job_done", C.c_void_p),
        ("ctl", C.c_void_p), ("reserved", C.c_int64 * 4),
    ]


class PlayEndgameMovesArgs(C.Structure):
    """Mirror of iago_play_endgame_moves_args (include/iago_hip_serving.h)."""
    _fields_ = [("play", PlayEndgameArgs), ("rec_best", C.c_void_p), ("reserved", C.c_int64 * 4)]


ALPHABETA_MAX_DEPTH = 10   # IAGO_ALPHABETA_MAX_DEPTH


class AlphaBetaArgs(C.Structure):
    """Mirror of iago_alphabeta_args (include/iago_hip_serving.h)."""
    _fields_ = [
        ("own", C.c_void_p), ("opp", C.c_void_p), ("n", C.c_int64),
        ("depth", C.c_int32), ("time_limit_ms", C.c_int32),
        ("score", C.c_void_p), ("move", C.c_void_p), ("nodes", C.c_void_p), ("done", C.c_void_p),
        ("ctl", C.c_void_p), ("reserved", C.c_int64 * 4),
    ]


ALPHABETA_MAX_SPLIT = 2         # IAGO_ALPHABETA_MAX_SPLIT
ALPHABETA_SPLIT_CTL_WORDS = 8   # IAGO_ALPHABETA_SPLIT_CTL_WORDS


class AlphaBetaSplitArgs(C.Structure):
    """Mirror of iago_alphabeta_split_args (include/iago_hip_serving.h)."""
    _fields_ = [
        ("own", C.c_void_p), ("opp", C.c_void_p), ("n", C.c_int64),
        ("depth", C.c_int32), ("split", C.c_int32), ("time_limit_ms", C.c_int32), ("reserved0", C.c_int32),
        ("score", C.c_void_p), ("move", C.c_void_p), ("nodes", C.c_void_p), ("done", C.c_void_p),
        ("job_count", C.c_void_p), ("job_first", C.c_void_p), ("job_capacity", C.c_int64),
        ("job_own", C.c_void_p), ("job_opp", C.c_void_p), ("job_root", C.c_void_p), ("job_path", C.c_void_p),
        ("job_score", C.c_void_p), ("job_move", C.c_void_p), ("job_nodes", C.c_void_p), ("job_done", C.c_void_p),
        ("ctl", C.c_void_p), ("reserved", C.c_int64 * 4),
    ]


class SearchParkArgs(C.Structure):
    """Mirror of iago_search_park_args (include/iago_hip_serving.h)."""
    _fields_ = [
        ("park_empties", C.c_int32), ("reserved0", C.c_int32), ("parked", C.c_void_p), ("stones", C.c_void_p),
        ("pass_flg", C.c_void_p), ("streams", C.c_void_p), ("reserved", C.c_int64 * 4),
    ]


class SearchExploreArgs(C.Structure):
    """Mirror of iago_search_explore_args (include/iago_hip_serving.h)."""
    _fields_ = [
        ("explore_turns", C.c_int32), ("reserved0", C.c_int32), ("streams", C.c_void_p), ("park", C.c_void_p),
        ("reserved", C.c_int64 * 4),
    ]


class SearchCapArgs(C.Structure):
    """Mirror of iago_search_cap_args (include/iago_hip_serving.h)."""
    _fields_ = [
        ("n_fast", C.c_int32), ("full_per_256", C.c_int32), ("explore_turns", C.c_int32), ("reserved0", C.c_int32),
        ("streams", C.c_void_p), ("park", C.c_void_p), ("reserved", C.c_int64 * 4),
    ]


class RootNoise(C.Structure):
    """Mirror of iago_root_noise (include/iago_hip_serving.h)."""
    _fields_ = [
        ("alpha_256", C.c_int32), ("eps_256", C.c_int32), ("draws", C.c_int32), ("reserved0", C.c_int32),
        ("counts", C.c_void_p),
    ]


class SearchNoiseArgs(C.Structure):
    """Mirror of iago_search_noise_args (include/iago_hip_serving.h)."""
    _fields_ = [
        ("noise", RootNoise), ("streams", C.c_void_p), ("reserved", C.c_int64 * 4),
    ]


class SearchForcedArgs(C.Structure):
    """Mirror of iago_search_forced_args (include/iago_hip_serving.h)."""
    _fields_ = [
        ("noise", RootNoise), ("streams", C.c_void_p), ("k_256", C.c_int32), ("reserved0", C.c_int32),
        ("reserved", C.c_int64 * 4),
    ]


class GumbelRoot(C.Structure):
    """Mirror of iago_gumbel_root (include/iago_hip_serving.h)."""
    _fields_ = [
        ("gumbel_q16", C.c_void_p), ("ln_q16", C.c_void_p), ("sched", C.c_void_p), ("g", C.c_void_p),
        ("m", C.c_int32), ("c_scale_256", C.c_int32), ("c_visit", C.c_int32), ("reserved0", C.c_int32),
    ]


class SearchGumbelArgs(C.Structure):
    """Mirror of iago_search_gumbel_args (include/iago_hip_serving.h)."""
    _fields_ = [
        ("gumbel", GumbelRoot), ("streams", C.c_void_p), ("reserved", C.c_int64 * 4),
    ]


class ValueSplitArgs(C.Structure):
    """Mirror of iago_value_split_args (include/iago_hip.h)."""
    _fields_ = [
        ("planes", C.c_void_p), ("own", C.c_void_p), ("opp", C.c_void_p), ("n", C.c_int64),
        ("w1", C.c_void_p), ("b1", C.c_void_p),
        ("w_hi", C.c_void_p * 7), ("w_lo", C.c_void_p * 7), ("bias", C.c_void_p * 7),
        ("w9_hi", C.c_void_p), ("w9_lo", C.c_void_p),
        ("b9", C.c_void_p), ("w10", C.c_void_p), ("w11", C.c_void_p),
        ("out", C.c_void_p), ("overflow", C.c_void_p), ("index", C.c_void_p), ("n_dev", C.c_void_p),
    ]


class MctsTree(C.Structure):
    """Mirror of iago_mcts_tree (include/iago_hip.h)."""
    _fields_ = [
        ("n_games", C.c_int64), ("capacity", C.c_int32), ("has_v", C.c_int32),
        ("nodes", C.c_void_p), ("n_nodes", C.c_void_p), ("root", C.c_void_p), ("overflow", C.c_void_p),
    ]


NODE_WORDS = 8   # sizeof(iago_mcts_node) / 4: n_visits, q, p, v, first_child, parent, action | n_children << 8, reserved


_lib = None
ABI_VERSION = 13   # iago_abi_version() of the include/iago_hip.h these bindings mirror


def lib():
    """The loaded library.  Raises IagoError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise IagoError(
            "iago_amd/libiago_hip.so is missing: run `python -m iago_amd.build` "
            "(or __graft_entry__.build()).  There is no CPU fallback.")
    # One HIP runtime per process: PyTorch bundles its own libamdhip64 (same
    # SONAME as /opt/rocm's).  Load torch's copy first so that this library's
    # NEEDED libamdhip64.so.7 binds to it instead of pulling in a second runtime
    # (two runtimes in one process: "no ROCm-capable device is detected").
    try:
        import torch
        bundled = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
        if os.path.exists(bundled):
            C.CDLL(bundled, mode=C.RTLD_GLOBAL)
    except ImportError:  # C-only hosts use the system runtime through RUNPATH
        pass
    L = C.CDLL(SO_PATH)
    vp, i64 = C.c_void_p, C.c_int64
    L.iago_abi_version.restype = C.c_int
    if L.iago_abi_version() != ABI_VERSION:
        # the ctypes structures below mirror ONE version of include/iago_hip.h
        raise IagoError("%s has ABI version %d, these bindings are for %d: rebuild it "
                        "(`python -m iago_amd.build`)" % (SO_PATH, L.iago_abi_version(), ABI_VERSION))
    L.iago_last_error.restype = C.c_char_p
    L.iago_device_count.restype = C.c_int
    L.iago_legal_moves.argtypes = [vp, vp, vp, i64, vp]
    L.iago_apply_moves.argtypes = [vp, vp, vp, i64, vp]
    L.iago_play_turn.argtypes = [vp, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, i64, vp]
    L.iago_encode_planes.argtypes = [vp, vp, vp, i64, vp]
    L.iago_encode_planes_indexed.argtypes = [vp, vp, vp, vp, i64, vp, vp]
    L.iago_judge.argtypes = [vp, vp, vp, i64, vp]
    L.iago_sample_moves.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, vp,
                                    i64, vp]
    L.iago_augment8.argtypes = [vp, vp, vp, vp, vp, vp, i64, vp]
    L.iago_bias_relu.argtypes = [vp, vp, i64, C.c_int32, vp]
    i32 = C.c_int32
    L.iago_conv3x3_split.argtypes = [vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, vp, vp]
    L.iago_conv3x3_split_trunk.argtypes = [C.POINTER(ConvSplitLayer), i32, i64, vp, vp]
    L.iago_value_forward_split.argtypes = [C.POINTER(ValueSplitArgs), vp]
    L.iago_policy_forward_split3.argtypes = [C.POINTER(PolicySplit3Args), vp]
    L.iago_value_rollout.argtypes = [C.POINTER(ValueSplitArgs), C.POINTER(RolloutArgs), vp]
    L.iago_conv3x3_wgrad_split.argtypes = [vp, vp, vp, vp, i64, i32, vp, i32, vp, vp, vp]
    L.iago_conv3x3_bwd_data_split.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, i64, vp]
    L.iago_split_scaled.argtypes = [vp, vp, vp, vp, vp, i64, i32, vp, vp, vp]
    L.iago_policy_grad_workspace_bytes.argtypes = [i64]
    L.iago_policy_grad_workspace_bytes.restype = i64
    L.iago_policy_reinforce_grad.argtypes = [C.POINTER(PolicyGradArgs), vp]
    L.iago_adam_chainer.argtypes = [C.POINTER(AdamArgs), vp]
    L.iago_value_grad_workspace_bytes.argtypes = [i64]
    L.iago_value_mse_grad.argtypes = [C.POINTER(ValueGradArgs), vp]
    L.iago_policy_visits_grad.argtypes = [C.POINTER(PolicyVisitsGradArgs), vp]
    L.iago_replay_sample.argtypes = [C.POINTER(ReplaySampleArgs), vp]
    L.iago_canonical_rows.argtypes = [vp, vp, i64, vp, vp, vp, vp]
    L.iago_replay_merge.argtypes = [C.POINTER(ReplayMergeArgs), vp]
    L.iago_replay_sample_merged.argtypes = [C.POINTER(ReplaySampleMergedArgs), vp]
    L.iago_value_targets.argtypes = [C.POINTER(ValueTargetsArgs), vp]
    L.iago_replay_merge_values.argtypes = [C.POINTER(ReplayMergeValuesArgs), vp]
    L.iago_split_nchw.argtypes = [vp, vp, vp, i64, i32, vp, vp]
    L.iago_merge_nchw.argtypes = [vp, vp, vp, i64, i32, vp]
    L.iago_value_stem.argtypes = [vp, vp, vp, vp, vp, i64, vp, vp]
    L.iago_value_stem_boards.argtypes = [vp, vp, vp, vp, vp, vp, i64, vp, vp]
    L.iago_value_head.argtypes = [vp, vp, vp, vp, vp, vp, vp, i64, vp]
    L.iago_conv3x3_f32.argtypes = [vp, vp, vp, vp, i64, i32, i32, vp, vp]
    L.iago_stem_f32.argtypes = [vp, vp, vp, vp, i64, vp, vp]
    L.iago_stem_f32_boards.argtypes = [vp, vp, vp, vp, vp, vp, i64, vp, vp]
    L.iago_policy_head.argtypes = [vp, vp, vp, vp, i64, vp, vp]
    L.iago_rollout_build_table.argtypes = [vp, vp, vp]
    L.iago_rollout.argtypes = [C.POINTER(RolloutArgs), vp]
    tp = C.POINTER(MctsTree)
    L.iago_mcts_reset.argtypes = [tp, vp, vp]
    L.iago_mcts_select.argtypes = [tp, vp, vp, vp, C.c_float, C.c_int32, C.c_int, vp, vp, vp, vp,
                                   vp, vp, vp]
    L.iago_mcts_expand.argtypes = [tp, vp, i64, vp, vp, vp, vp, vp]
    L.iago_leaf_values.argtypes = [vp, vp, C.c_float, vp, i64, vp]
    L.iago_mcts_backup.argtypes = [tp, vp, vp, vp, vp]
    L.iago_mcts_mix_backup.argtypes = [tp, vp, vp, vp, vp, C.c_float, vp, vp, vp]
    L.iago_mcts_pending.argtypes = [vp, vp, i64, vp, vp, vp, vp, vp, vp]
    L.iago_mcts_best_move.argtypes = [tp, vp, vp, vp, vp]
    L.iago_mcts_root_value.argtypes = [tp, vp, vp, vp, vp, vp]
    L.iago_mcts_advance_root.argtypes = [tp, vp, vp, vp]
    L.iago_mcts_compact.argtypes = [tp, tp, vp, vp, vp]
    lp = C.POINTER(MctsLookahead)
    L.iago_mcts_mix_backup_lookahead.argtypes = [tp, vp, vp, vp, vp, vp, vp, C.c_float, vp, vp, lp, vp]
    L.iago_mcts_store_priors.argtypes = [lp, vp, vp, vp]
    L.iago_mcts_expand_cached.argtypes = [tp, vp, vp, vp, vp, lp, vp, vp]
    L.iago_mcts_fresh_leaves.argtypes = [tp, vp, vp, vp, vp, vp, vp]
    L.iago_mcts_descend.argtypes = [tp, vp, vp, vp, C.c_float, i32, vp, vp, vp, vp, vp, lp, vp, vp, vp, vp]
    L.iago_value_forward_batch.argtypes = [C.POINTER(ValueSplitArgs), i32, i32, vp]
    vap = C.POINTER(MctsValueAhead)
    L.iago_mcts_value_ahead_rows.argtypes = [tp, vap, vp]
    L.iago_mcts_value_ahead_store.argtypes = [tp, vap, vp]
    L.iago_mcts_search_persistent.argtypes = [C.POINTER(MctsSearchArgs), vp]
    L.iago_mcts_search_capacity.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.iago_mcts_search_streams_create.argtypes = [i32, C.POINTER(vp)]
    L.iago_mcts_search_streams_destroy.argtypes = [vp]
    L.iago_mcts_search_split.argtypes = [C.POINTER(MctsSearchArgs), vp, vp]
    L.iago_mcts_search_wave.argtypes = [C.POINTER(MctsSearchArgs), C.POINTER(SearchWaveArgs), vp]
    L.iago_selfplay_policy.argtypes = [C.POINTER(SelfplayPolicyArgs), vp]
    L.iago_solve_endgame.argtypes = [C.POINTER(EndgameArgs), vp]
    L.iago_play_endgame.argtypes = [C.POINTER(PlayEndgameArgs), vp]
    L.iago_solve_endgame_moves.argtypes = [C.POINTER(EndgameMovesArgs), vp]
    L.iago_play_endgame_moves.argtypes = [C.POINTER(PlayEndgameMovesArgs), vp]
    L.iago_mcts_search_park.argtypes = [C.POINTER(MctsSearchArgs), C.POINTER(SearchParkArgs), vp]
    L.iago_mcts_search_explore.argtypes = [C.POINTER(MctsSearchArgs), C.POINTER(SearchExploreArgs), vp]
    L.iago_mcts_draw_move.argtypes = [tp, vp, C.c_uint64, vp, vp, vp, vp, vp]
    L.iago_mcts_search_cap.argtypes = [C.POINTER(MctsSearchArgs), C.POINTER(SearchCapArgs), vp]
    L.iago_mcts_cap_mask.argtypes = [C.c_uint64, vp, vp, i32, i64, vp, vp]
    L.iago_mcts_root_noise.argtypes = [tp, vp, vp, vp, C.c_uint64, vp, vp, C.POINTER(RootNoise), vp]
    L.iago_mcts_search_noise.argtypes = [C.POINTER(MctsSearchArgs), C.POINTER(SearchNoiseArgs), vp]
    L.iago_mcts_search_forced.argtypes = [C.POINTER(MctsSearchArgs), C.POINTER(SearchForcedArgs), vp]
    L.iago_mcts_gumbel_draw.argtypes = [tp, vp, C.c_uint64, vp, vp, C.POINTER(GumbelRoot), vp]
    L.iago_mcts_search_gumbel.argtypes = [C.POINTER(MctsSearchArgs), C.POINTER(SearchGumbelArgs), vp]
    L.iago_mcts_gumbel_finish.argtypes = [tp, vp, C.POINTER(GumbelRoot), vp, vp, vp, vp, vp]
    L.iago_mcts_prune_visits.argtypes = [tp, vp, C.c_float, i32, vp, vp]
    L.iago_mcts_prune_visits_rule.argtypes = [tp, vp, C.c_float, i32, i32, vp, vp]
    L.iago_mcts_search_arena.argtypes = [C.POINTER(MctsSearchArgs), C.POINTER(MctsSearchArgs), vp]
    L.iago_alphabeta_moves.argtypes = [C.POINTER(AlphaBetaArgs), vp]
    L.iago_alphabeta_moves_split.argtypes = [C.POINTER(AlphaBetaSplitArgs), vp]
    L.iago_solve_endgame_split.argtypes = [C.POINTER(EndgameSplitArgs), vp]
    L.iago_random_moves.argtypes = [vp, vp, i64, C.c_uint64, C.c_uint32, C.c_uint32, i32, vp, vp]
    for name in SYMBOLS[3:] + LAYER_SYMBOLS + EXPERIMENTAL_SYMBOLS + SERVING_SYMBOLS + TRAINING_SYMBOLS:
        getattr(L, name).restype = C.c_int
    L.iago_policy_grad_workspace_bytes.restype = i64   # (bytes: beyond 2^31 from ~7,000 rows on)
    L.iago_value_grad_workspace_bytes.restype = i64
    _lib = L
    return L


def check(rc, what=""):
    if rc != IAGO_OK:
        msg = lib().iago_last_error().decode("utf-8", "replace")
        raise IagoError("%s failed (%d): %s" % (what or "iago call", rc, msg))


def device_count():
    return lib().iago_device_count()
