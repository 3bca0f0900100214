/*
 * iago_hip_serving.h -- searching ONE position fast: the entry points that serve a single game (MCTS.get_move behind
 * the front end) rather than batches of games.  Same conventions as iago_hip.h; part of the library's ABI
 * (iago_abi_version).
 */
#ifndef IAGO_HIP_SERVING_H
#define IAGO_HIP_SERVING_H

#include "iago_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct iago_search_wave_args {
    int32_t width;   /* W: playouts of one tree in flight together, 1, 8, 16 or 32 */
    float vloss;     /* virtual loss of an in-flight visit, >= 0 (1.0: counted as a loss; 0: only the counts steer) */
    int64_t *timing; /* optional [4] int64, added to (100 MHz ticks summed over the game workgroups): descents, rollout
                        passes, backups, iterations in which every slot waited for a net */
    int64_t reserved[4];
} iago_search_wave_args;

/*
 * The persistent search of iago_mcts_search_persistent with W playouts of every tree in flight at once.
 * Tree g owns the W consecutive SLOTS g*W .. g*W+W-1; every array of `args` that is per game there is per slot here
 * ([n_games*W]: cur_node, cur_own, cur_opp, done, roll, leaf_value, rep_v; rep_p [n_games*W*64]; path
 * [n_games*W][path_stride]; the rollout's n = n_games*W), the rest stays per tree (root_own, root_opp, active, the
 * tree, z_log_n, z_log [rows][n_games], stats).  A search of n_sims playouts runs as ceil(n_sims / W) WAVES (the last
 * one n_sims mod W playouts, or W); playout p is slot p mod W of wave p div W.  Every tree node counts its in-flight
 * visits in `reserved1` (vv, 0 outside a wave; every node-creating path leaves it 0):
 *   - the descents of a wave run one after the other in slot order, each exactly MCTS.playout's (expansion when the
 *     real n_visits >= n_thr, the priors at the expansion, first maximum wins) except that child c of parent X scores
 *     Q_eff + float32(c_puct * P) * sqrt(X.n + X.vv) / (0.01 + c.n + c.vv) in float64, Q_eff = c.Q when c.vv == 0,
 *     else (c.Q * c.n - vloss * c.vv) / (c.n + c.vv); a descent that reaches its leaf adds 1 to vv along its path;
 *   - a leaf is evaluated as before (value cache, position table, value net; the rollout draws from Philox stream
 *     rollout->stream_id + p with id_base + g), as soon as its descent ends;
 *   - when all leaves of the wave are evaluated the backups run in slot order: vv -= 1 along the path, then the
 *     reference's update.  z_log is written in playout order.
 * With W = 1 every vv stays 0: the trees, moves, z_log and draws of iago_mcts_search_persistent, bit for bit.
 * The game workgroups hold 32 slots each (games_per_workgroup is not read).  Whole games are not available here:
 * max_turns > 0 or games_total > 0 is refused, as is a width outside {1, 8, 16, 32} or a negative / NaN vloss
 * (IAGO_ERR_INVALID).  ctl[3] != 0 after the launch: it gave up, and the trees' vv are NOT 0 (reset them).
 */
IAGO_API int iago_mcts_search_wave(const iago_mcts_search_args *args, const iago_search_wave_args *wave, void *stream);

/*
 * The negamax backup: OR-ed into iago_mcts_search_args.games_per_workgroup (a positive one, like
 * IAGO_SEARCH_CHAIN_SKIP; both are stripped before the number is read), for every entry point that takes those
 * arguments -- the single launch, the role split, whole games, streams and matches, park / explore / cap / noise /
 * forced, the wave search, and each argument set of iago_mcts_search_arena on its own (A and B may differ).
 * Without it a playout's leaf value lv (leaf_mix of the value net and the rollout, both from the leaf mover's view) is
 * added unchanged to every node of the path, the reference's Node.update_recursive.  With it a node's Q is the value
 * from the view of the player who moved INTO the node: of the path node[0] (the root) .. node[L] (the leaf), node[d]
 * is visited with +lv where L - d is odd and with -lv where it is even -- update_recursive starting with -lv at the
 * leaf and negating once per parent.  A pass is a move: pass children are levels like any other.  The negation is
 * exact and Node.update's arithmetic is unchanged.  leaf_value[], z_log, the stored values (node.v, the position
 * table, values walked ahead), the selection rule, forced playouts and their pruning, the wave search's virtual loss
 * and the moves read from the visit counts are untouched; the root's own Q plays no part in selection.
 * The per-playout launches (iago_mcts_mix_backup_lookahead, iago_mcts_mix_backup, iago_mcts_backup) keep the
 * reference's rule.
 */
#define IAGO_SEARCH_NEGAMAX 0x200

/*
 * The AlphaZero selection rule: OR-ed into iago_mcts_search_args.games_per_workgroup (a positive one, like
 * IAGO_SEARCH_CHAIN_SKIP and IAGO_SEARCH_NEGAMAX; all three are stripped before the number is read), for every entry
 * point that takes those arguments -- the single launch, the role split, whole games, streams and matches, park /
 * explore / cap / noise / forced, the wave search, and each argument set of iago_mcts_search_arena on its own (A and B
 * may differ).  Without it the search selects by the reference's formula.  With it, two changes and no others:
 *   1. The stored prior.  A child created by Node.expand for move a stores float32(prob[a]); the reference stores
 *      float32(float32(prob[a]) + float32(0.1)).  The single-move child and the pass child (Node(node, 1.0) without a
 *      net) store 1.0, not 1.1.  A root created as Node(None, 1.0) -- iago_mcts_reset (which takes no flags), a game's
 *      start inside a launch, a stream's next game, a move that is no child of the root -- stores 1.1 under BOTH rules: a
 *      root's prior is never read.  A root reached by subtree reuse is a former child and keeps what it stored.
 *   2. The score.  Q + float64(float32(c_puct * P)) * sqrt(float64(N_parent)) / (1.0 + n) in float64, every operation
 *      rounded on its own; the reference divides by 0.01 + n.  The wave search's denominator is 1.0 + n + vv, its Q_eff
 *      unchanged.  An unvisited child's Q stays 0; the first maximum still wins.
 * Expansion at n_thr, the leaf mix, both backup rules, the value cache and the position table, the pass-chain skip and
 * the move read from the visit counts are untouched.  Root noise mixes the STORED prior as it stands (the mix's own
 * arithmetic is unchanged), so under this rule it is p (1 - eps) + eps c / N on the policy's p; a forced child is judged
 * by its STORED prior as it stands, n < sqrt(k p N) on the (mixed) policy's p.  The pruning scores with the rule's
 * denominator: iago_mcts_prune_visits_rule.
 * The per-playout launches (iago_mcts_select, iago_mcts_expand and their kin) keep the reference's rule.
 */
#define IAGO_SEARCH_PUCT_AZ 0x400

/* ------------------------------------------------------------------ exact endgame */

#define IAGO_ENDGAME_EXACT 0          /* mode: the exact final disc difference */
#define IAGO_ENDGAME_WLD 1            /* mode: its sign only (win / draw / loss) */
#define IAGO_ENDGAME_MAX_EMPTIES 20   /* the largest max_empties */
#define IAGO_ENDGAME_MAX_TIME_MS 600000
#define IAGO_ENDGAME_CTL_WORDS 4

typedef struct iago_endgame_args {
    const uint64_t *own; /* [n] side to move (bit a = row*8+col) */
    const uint64_t *opp; /* [n] its opponent */
    int64_t n;
    int32_t mode;          /* IAGO_ENDGAME_EXACT or IAGO_ENDGAME_WLD */
    int32_t max_empties;   /* 0 .. IAGO_ENDGAME_MAX_EMPTIES: sizes the search stack */
    int32_t time_limit_ms; /* 1 .. IAGO_ENDGAME_MAX_TIME_MS: the launch gives up after this long on the device clock */
    int32_t reserved0;     /* 0 */
    int8_t *score;         /* [n] out */
    int8_t *move;          /* [n] out */
    int64_t *nodes;        /* [n] out: nodes visited */
    uint8_t *solved;       /* [n] out: 1 = score and move are exact */
    uint32_t *ctl;         /* [IAGO_ENDGAME_CTL_WORDS] cleared by the call; [0] != 0: gave up, [2]: positions refused */
    int64_t reserved[4];   /* 0 */
} iago_endgame_args;

/*
 * The exact value of n Othello positions under perfect play, one lane per position (negamax alpha-beta, no tables).
 * Rules are the library's: a side with no legal move passes, the game ends when neither side can move (a full board
 * included), and the score is #own - #opp at the end, empty squares counted for nobody (judge's count, so
 * sign(score) is the reference's result z for the side to move).
 *   - EXACT: score[i] = the negamax value in [-64, 64]; move[i] = the LOWEST-indexed move that reaches it (the
 *     reference's first-maximum order).
 *   - WLD: score[i] = its sign, found with a window (-1, 1) around 0 (much cheaper); move[i] = the lowest-indexed move
 *     that reaches that outcome.
 *   - move[i] is -1 when the side to move must pass, -2 when the game is over; nodes[i] counts the nodes visited.
 * A position with own & opp != 0 or with more than max_empties empties is refused: solved[i] = 0, ctl[2] counts it.
 * solved[] and ctl are cleared on `stream` before the launch, and score / move / nodes are meaningful where
 * solved[i] = 1.  The launch stops on its own clock after time_limit_ms: then ctl[0] != 0 and every position it had
 * not finished keeps solved[i] = 0, so a launch never hangs the device whatever it is given.  Host-side refusals
 * (IAGO_ERR_INVALID, nothing launched): a null args / ctl, a null array with n > 0, n < 0, a mode outside the two, a
 * max_empties or time_limit_ms out of range, reserved fields not 0.
 */
IAGO_API int iago_solve_endgame(const iago_endgame_args *args, void *stream);

typedef struct iago_play_endgame_args {
    uint64_t *own;           /* [n] in: the position at the game's turn, own = the side to move; out: the final position,
                                own = the side that would move next (colour 1 after an even number of turns) */
    uint64_t *opp;           /* [n] in / out */
    int32_t *turn;           /* [n] in: the turn the game stands at, 0 .. max_turns - 1; out: the turns it took */
    const int32_t *stones;   /* [n] the game's stone count (game.py:32: 4 at the start, + 1 per move) */
    const uint8_t *pass_flg; /* [n] the turn before this one was a pass */
    const uint8_t *parked;   /* [n] 1: play this game; 0: not touched (finished stays 0) */
    int64_t n;
    int64_t stride;          /* >= n: the records' row of turn t and game g is t * stride + g */
    int32_t max_turns;       /* 1 .. IAGO_MAX_TURNS: the records' rows; a game ends there at the latest */
    int32_t max_empties;     /* 0 .. IAGO_ENDGAME_MAX_EMPTIES: sizes the search stack; a game with more empties is refused */
    int32_t time_limit_ms;   /* 1 .. IAGO_ENDGAME_MAX_TIME_MS */
    int32_t reserved0;       /* 0 */
    uint64_t *rec_own;       /* [max_turns][stride] out: the position before the turn (own = mover) */
    uint64_t *rec_opp;
    uint8_t *rec_valid;      /* 3: a solved move; 0: a pass or no turn */
    int8_t *rec_move;        /* the move played, -1 = pass / no turn */
    int8_t *rec_score;       /* the exact final disc difference from the mover's view (0 where valid is 0) */
    uint8_t *finished;       /* [n] out: 1 = the game was played to its end */
    uint32_t *ctl;           /* [IAGO_ENDGAME_CTL_WORDS] cleared by the call; [0] != 0: gave up, [2]: games refused */
    int64_t reserved[4];     /* 0 */
} iago_play_endgame_args;

/*
 * The parked games of a batch (parked[g] = 1) to their end under perfect play, one lane per game, each on its own clock:
 * at every turn the mover's position is solved as iago_solve_endgame does in mode EXACT (same search, same move: the
 * lowest-indexed one that reaches the best final disc difference) and the move is played with the books of the whole-game
 * search (iago_mcts_search_persistent with max_turns > 0; game.py:117-142,253-255): a stone per move, a pass when the
 * mover has no move, a pass after a pass sets stones = 64, `stones >= 64` is tested after odd turns only, and the game
 * ends at an even turn or at max_turns.  Every turn from the game's `turn` on writes its row of the records; rows before
 * it and rows of other games are not touched.  At the end turn / own / opp hold the game's turn count and final position
 * and finished[g] = 1.  A game with own & opp != 0, more than max_empties empties or a turn outside 0 .. max_turns - 1 is
 * refused (finished[g] = 0, ctl[2] counts it, nothing else written).  finished[] and ctl are cleared on `stream` before
 * the launch; it stops on its own clock after time_limit_ms (ctl[0] != 0, the unfinished games keep finished = 0 and
 * their turn / own / opp).  Host-side refusals (IAGO_ERR_INVALID, nothing launched): a null args / ctl, a null array
 * with n > 0, n < 0, stride < n, max_turns, max_empties or time_limit_ms out of range, reserved fields not 0.
 */
IAGO_API int iago_play_endgame(const iago_play_endgame_args *args, void *stream);

#define IAGO_ENDGAME_MOVES_BEST 0  /* moves: the set of the optimal moves */
#define IAGO_ENDGAME_MOVES_ALL 1   /* moves: that set and the value of every legal move */
#define IAGO_ENDGAME_NO_MOVE (-128) /* move_score: the cell is no legal move of the mover */

typedef struct iago_endgame_moves_args {
    const uint64_t *own; /* [n] side to move (bit a = row*8+col) */
    const uint64_t *opp; /* [n] its opponent */
    int64_t n;
    int32_t mode;          /* IAGO_ENDGAME_EXACT or IAGO_ENDGAME_WLD */
    int32_t moves;         /* IAGO_ENDGAME_MOVES_BEST or IAGO_ENDGAME_MOVES_ALL */
    int32_t max_empties;   /* 0 .. IAGO_ENDGAME_MAX_EMPTIES: sizes the search stack */
    int32_t time_limit_ms; /* 1 .. IAGO_ENDGAME_MAX_TIME_MS: the launch gives up after this long on the device clock */
    int8_t *score;         /* [n] out */
    int8_t *move;          /* [n] out: the lowest set bit of best[i]; -1: the mover must pass, -2: the game is over */
    int64_t *nodes;        /* [n] out: nodes visited */
    uint8_t *solved;       /* [n] out: 1 = the outputs of position i are exact */
    uint64_t *best;        /* [n] out: bit a set iff move a reaches score[i] */
    int8_t *move_score;    /* [n][64] out, ALL only (NULL under BEST): the value of move a from the mover's view */
    uint32_t *ctl;         /* [IAGO_ENDGAME_CTL_WORDS] cleared by the call; [0] != 0: gave up, [2]: positions refused */
    int64_t reserved[4];   /* 0 */
} iago_endgame_moves_args;

/*
 * iago_solve_endgame with EVERY optimal move, and under ALL every move's value.  Same search, same move order, same
 * rules of the game; score[i] and move[i] are iago_solve_endgame's, bit for bit, in both modes.  The root differs:
 *   - BEST: after the first move every move of the root is searched with alpha = max(alpha, best - 1), whatever its
 *     index, so every move that ties the best value comes back exact.  best[i] has bit a set iff move a reaches
 *     score[i] (under WLD: reaches that outcome -- after a win is found the other moves are still searched, with the
 *     window (0, 1)).  About 1.1 x the nodes of iago_solve_endgame in mode EXACT.
 *   - ALL: the root's alpha never rises: every legal move is searched with the full window (-65, 65) (WLD: (-1, 1)),
 *     move_score[i][a] is its exact value from the mover's view (WLD: its sign), IAGO_ENDGAME_NO_MOVE on every cell
 *     that is no legal move of the mover; best[i] is the argmax.  nodes[i] is the root plus what each child's
 *     full-window search visits.  About 2.2 x the nodes.
 *   - a root that must pass is a node like any other: move -1, best 0, the whole row IAGO_ENDGAME_NO_MOVE; a finished
 *     game: move -2, best 0, the whole row IAGO_ENDGAME_NO_MOVE; a root with one empty: its move is the set and that
 *     move's value the score.
 * A position with own & opp != 0 or with more than max_empties empties is refused: solved[i] = 0, best[i] = 0, its row
 * IAGO_ENDGAME_NO_MOVE, ctl[2] counts it.  solved[], ctl and move_score are cleared on `stream` before the launch;
 * score / move / nodes / best / move_score are meaningful where solved[i] = 1.  The clock (ctl[0]) and the stack
 * overflow word (ctl[3]) are iago_solve_endgame's.  Host-side refusals (IAGO_ERR_INVALID, nothing launched): a null
 * args / ctl, a null array with n > 0, n < 0, a mode or a `moves` outside the two, move_score given under BEST or
 * missing under ALL, a max_empties or time_limit_ms out of range, reserved fields not 0.
 */
IAGO_API int iago_solve_endgame_moves(const iago_endgame_moves_args *args, void *stream);

#define IAGO_ENDGAME_MAX_SPLIT 2
#define IAGO_ENDGAME_SPLIT_CTL_WORDS 8

typedef struct iago_endgame_split_args {
    const uint64_t *own; /* [n] side to move (bit a = row*8+col) */
    const uint64_t *opp; /* [n] its opponent */
    int64_t n;           /* at most 2^31 - 1 */
    int32_t mode;          /* IAGO_ENDGAME_EXACT or IAGO_ENDGAME_WLD */
    int32_t split;         /* 1 .. IAGO_ENDGAME_MAX_SPLIT: the plies expanded into jobs */
    int32_t max_empties;   /* 0 .. IAGO_ENDGAME_MAX_EMPTIES: sizes the search stack; a root with more empties is refused */
    int32_t time_limit_ms; /* 1 .. IAGO_ENDGAME_MAX_TIME_MS, of the search stage */
    int8_t *score;         /* [n] out */
    int8_t *move;          /* [n] out */
    int64_t *nodes;        /* [n] out */
    uint8_t *solved;       /* [n] out: 1 = every job of the root finished, the outputs of root i are exact */
    uint64_t *best;        /* [n] out, or NULL (not wanted): bit a set iff move a reaches score[i] */
    int8_t *move_score;    /* [n][64] out, or NULL (not wanted): the value of move a from the mover's view */
    int32_t *job_count;    /* [n] out: the jobs of root i */
    int64_t *job_first;    /* [n] out: the index of its first job (the exclusive sum of job_count) */
    int64_t job_capacity;  /* the jobs the arrays below hold, at most 2^31 - 1 */
    uint64_t *job_own;     /* [job_capacity] out: the job's side to move */
    uint64_t *job_opp;     /* [job_capacity] out */
    int32_t *job_root;     /* [job_capacity] out: the root it belongs to */
    int8_t *job_path;      /* [job_capacity][4] out: the job's empties, first move, second move (-1 where absent), 0 */
    int8_t *job_score;     /* [job_capacity] out: iago_solve_endgame's score of (job_own, job_opp) */
    int8_t *job_move;      /* [job_capacity] out: its move */
    int64_t *job_nodes;    /* [job_capacity] out: its nodes */
    uint8_t *job_done;     /* [job_capacity] out */
    uint32_t *ctl;         /* [IAGO_ENDGAME_SPLIT_CTL_WORDS] cleared by the call; [0] != 0: gave up, [1]: the claim
                              counter, [2]: roots refused, [3] != 0: a stack overflow, [4] / [5]: the low / high word of
                              the jobs needed, [6] != 0: they exceed job_capacity (nothing was searched), [7]: 0 */
    int64_t reserved[4];   /* 0 */
} iago_endgame_split_args;

/*
 * iago_solve_endgame with every root's search spread over many lanes -- the solver's counterpart of
 * iago_alphabeta_moves_split below, with the same three stages, each a launch of its own on `stream` and no host round
 * trip between them: score[i], move[i] and solved[i] are iago_solve_endgame's, bit for bit, in both modes.  The rule: a
 * node (own, opp) with k split plies left (the root: split)
 *   - is a JOB when k == 0 or its mover has no legal move: its (score, move, nodes) are what iago_solve_endgame
 *     returns for that position in the launch's mode, found with the full window on a stack of its own empties;
 *   - is EXPANDED otherwise: its children are its legal moves in ascending index, each with k - 1, its value the
 *     maximum of the negated children's values.
 * So a root that must pass or whose game is over is its own job (move -1 / -2), a child that cannot move -- it must
 * pass, or the game is over -- is one job, and a root with fewer empties than split plies ends in finished-game jobs:
 * split never has to be below the empties.  move[i] is the lowest-indexed move whose value equals score[i]; nodes[i] =
 * the nodes expanded (1 for the root, 1 per expanded child; a root that is its own job: none) + the sum of its jobs'
 * nodes, so it depends on no timing.  Every first move of an expanded root has its exact value here, so two optional
 * outputs come for free, and equal iago_solve_endgame_moves' under BEST / ALL: best[i] = the set of the moves reaching
 * score[i]; move_score[i][a] = the value of move a, IAGO_ENDGAME_NO_MOVE on every other cell (the call fills the array
 * on `stream` before the launches).  A passing root, a finished game and a refused root: best 0, the whole row
 * IAGO_ENDGAME_NO_MOVE.
 * The stages: (1) the jobs of every root are counted (job_count), summed (job_first; ctl[4] / [5] = their total) and
 * written in canonical order -- root ascending, then first move, then second move; (2) the lanes of iago_solve_endgame's
 * search claim jobs one at a time; (3) a thread per root takes its run of jobs back, the sign turned once per ply of the
 * path.  More jobs than job_capacity: ctl[6] is set, nothing is searched, every solved[i] stays 0 and nothing is written
 * past the capacity.  The COUNT-ONLY form -- every job_* array null and job_capacity 0 -- writes job_count, job_first
 * and ctl[4] / [5] and launches nothing else (score, move, nodes, solved, best and move_score are not touched and may be
 * null; ctl[6] stays 0).  A root with own & opp != 0 or more than max_empties empties is refused: ctl[2] counts it, it
 * has no job, solved[i] = 0 (score, move, nodes and best 0).  The give-up is the search stage's: ctl[0] != 0, and a root
 * with an unfinished job keeps solved[i] = 0 and is not written.  Host-side refusals (IAGO_ERR_INVALID, nothing
 * launched): a null args / ctl / own / opp / job_count / job_first with n > 0, n < 0 or above 2^31 - 1, a mode outside
 * the two, a split outside 1 .. IAGO_ENDGAME_MAX_SPLIT, a max_empties or time_limit_ms out of range, a job_capacity below
 * 0 or above 2^31 - 1, some but not all job_* arrays null or null ones with a capacity, a null score / move / nodes /
 * solved outside the count-only form, reserved fields not 0.
 */
IAGO_API int iago_solve_endgame_split(const iago_endgame_split_args *args, void *stream);

typedef struct iago_play_endgame_moves_args {
    iago_play_endgame_args play; /* iago_play_endgame's arguments, read as it reads them */
    uint64_t *rec_best;          /* [max_turns][stride] out: the BEST set of every solved turn, 0 where valid is 0 */
    int64_t reserved[4];         /* 0 */
} iago_play_endgame_moves_args;

/*
 * iago_play_endgame with one more record: every turn that writes its row also writes rec_best, the set of the moves
 * that reach the turn's exact score (iago_solve_endgame_moves, EXACT, BEST), 0 on a pass or no turn.  The move played
 * is the set's lowest bit: iago_play_endgame's move, so every other output equals iago_play_endgame's bit for bit.
 * Refusals are iago_play_endgame's, and a null rec_best with n > 0.
 */
IAGO_API int iago_play_endgame_moves(const iago_play_endgame_moves_args *args, void *stream);

typedef struct iago_search_park_args {
    int32_t park_empties;         /* 0 .. IAGO_ENDGAME_MAX_EMPTIES */
    int32_t reserved0;            /* 0 */
    uint8_t *parked;              /* [games] out: 1 = the game was handed over (cleared by the call) */
    int32_t *stones;              /* [games] out, where parked: the game's stone count */
    uint8_t *pass_flg;            /* [games] out, where parked: the turn before was a pass */
    iago_search_streams *streams; /* optional: the role split of iago_mcts_search_split; NULL = the single launch */
    int64_t reserved[4];          /* 0 */
} iago_search_park_args;

/*
 * Whole self-play games (iago_mcts_search_persistent with max_turns > 0, a stream included) that HAND OVER at
 * park_empties: a game whose turn would be searched -- the mover can move and the game is not over -- at a position with
 * 64 - popcount(own | opp) <= park_empties runs no search there.  It writes n_turns (the turn it stands at), game_own /
 * game_opp (own = the mover), stones, pass_flg and parked = 1, all indexed by the game's id ([games] = games_total, or
 * n_games), and is done: its workgroup goes on as after a finished game (net work, or the stream's next game).  Its
 * records hold the turns before that one.  Everything before the hand-over is iago_mcts_search_persistent's, bit for
 * bit; iago_play_endgame plays the parked games to their end.  Refused (IAGO_ERR_INVALID): null args or outputs,
 * max_turns == 0, a park_empties outside 0 .. 20, reserved fields not 0, and match codes (2 / 3) in `active` -- the
 * policy side of a match needs the net workgroups to its last move; `active` is read back on `stream` for this check
 * when it is device memory (not in a stream, which does not read it).
 */
IAGO_API int iago_mcts_search_park(const iago_mcts_search_args *args, const iago_search_park_args *park, void *stream);

/* ------------------------------------------------------------------ exploring self-play */

#define IAGO_EXPLORE_KEY 0x4558504Cu /* ("EXPL") the draws' Philox key: the rollout seed with its high word XOR this */

typedef struct iago_search_explore_args {
    int32_t explore_turns;             /* 0 .. IAGO_MAX_TURNS: the turns (the game's turn counter, passes included) whose
                                          searched move is drawn; 0 = none */
    int32_t reserved0;                 /* 0 */
    iago_search_streams *streams;      /* optional: the role split of iago_mcts_search_split; NULL = the single launch */
    const iago_search_park_args *park; /* optional: the hand-over of iago_mcts_search_park in the same launch (its
                                          `streams` NULL or the one above) */
    int64_t reserved[4];               /* 0 */
} iago_search_explore_args;

/*
 * Whole self-play games (iago_mcts_search_persistent with max_turns > 0, a stream included) that EXPLORE in their first
 * explore_turns turns: at a searched turn t < explore_turns of the game with global id G (its index, a stream: its game
 * id) the move is not the most visited child but drawn in proportion to the root's visit counts, in integers:
 *   - n[a]: the visits of the root's children, the mover's legal moves in ascending cell order -- the turn's rec_pi row;
 *     N = sum n[a];
 *   - w: word t & 3 of Philox4x32-10 on the counter (rollout->id_base + G, t >> 2, 0, 0) under the key rollout->seed with
 *     its high word XOR IAGO_EXPLORE_KEY; r = (uint64(w) * N) >> 32;
 *   - the move is the lowest cell a with sum_{b <= a} n[b] > r (a cell without visits is never drawn).
 * N == 0 (children, none visited): the first maximum, as without the draw; no children: ctl[4] is raised as before.  The
 * record keeps its shape (valid 1, rec_pi the visit row, rec_move the drawn move) and the drawn child becomes the root.
 * Turns from explore_turns on, and everything with explore_turns = 0, are iago_mcts_search_persistent's (with `streams`
 * iago_mcts_search_split's, with `park` iago_mcts_search_park's), bit for bit.  Refused (IAGO_ERR_INVALID): null args, an
 * explore_turns outside 0 .. IAGO_MAX_TURNS, reserved fields not 0, a bad `park`, max_turns == 0, and match codes (2 / 3)
 * in `active` (read as iago_mcts_search_park reads it; not in a stream).
 */
IAGO_API int iago_mcts_search_explore(const iago_mcts_search_args *args, const iago_search_explore_args *explore, void *stream);

/*
 * iago_mcts_best_move's sibling for the turn loop: move[g] of every game with active[g] != 0 (active NULL: every game) is
 * drawn by the rule above from the children of its tree's root, with id game_id[g] (the GLOBAL id, id_base + G, as its 32
 * bits) and turn turn[g], under `seed` (the rollout seed; the XOR is applied here).  visits (optional [n_games][64]): the
 * root's visit counts by action, as iago_mcts_best_move writes them.  N == 0: the first maximum; no children: -2.
 * Refused (IAGO_ERR_INVALID): a bad tree, null game_id, turn or move.
 */
IAGO_API int iago_mcts_draw_move(const iago_mcts_tree *tree, const uint8_t *active, uint64_t seed, const int32_t *game_id,
                                 const int32_t *turn, int8_t *move, int32_t *visits, void *stream);

/* ------------------------------------------------------------------ playout-cap randomisation */

#define IAGO_CAP_KEY 0x43415050u /* ("CAPP") the cap's Philox key: the rollout seed with its high word XOR this */

typedef struct iago_search_cap_args {
    int32_t n_fast;                    /* 1 .. n_sims: the playouts of a fast turn */
    int32_t full_per_256;              /* 1 .. 256: a searched turn is full with probability full_per_256 / 256 */
    int32_t explore_turns;             /* 0 .. IAGO_MAX_TURNS: as iago_search_explore_args' (0 = no draw) */
    int32_t reserved0;                 /* 0 */
    iago_search_streams *streams;      /* optional: the role split of iago_mcts_search_split; NULL = the single launch */
    const iago_search_park_args *park; /* optional: the hand-over of iago_mcts_search_park in the same launch (its
                                          `streams` NULL or the one above) */
    int64_t reserved[4];               /* 0 */
} iago_search_cap_args;

/*
 * Whole self-play games (iago_mcts_search_persistent with max_turns > 0, a stream included) under PLAYOUT-CAP
 * RANDOMISATION: every searched turn t (the game's turn counter, passes included) of the game with global id G is FULL or
 * FAST, in integers:
 *   - w: word t & 3 of Philox4x32-10 on the counter (rollout->id_base + G, t >> 2, 0, 0) under the key rollout->seed with
 *     its high word XOR IAGO_CAP_KEY (a key of its own: not the explore draw's, a match's or the replay window's);
 *   - the turn is full iff (w >> 24) < full_per_256, else fast.
 * A full turn runs n_sims playouts and records valid 1; a fast turn runs n_fast playouts and records valid 4, rec_pi and
 * rec_move filled as for a full turn.  Playout p of turn t draws the rollout stream rollout->stream_id + t * n_sims + p on
 * both kinds of turn -- a fast turn is the first n_fast playouts of the full turn's search -- and `done`, the tree carried
 * to the next turn, the move (the most visited child; below explore_turns the draw of iago_mcts_search_explore) and the
 * books are iago_mcts_search_persistent's.  A fast root that ends without children raises ctl[4] as a full one does.
 * With full_per_256 = 256 every turn is full: that launch, bit for bit (`streams`: iago_mcts_search_split's, `park`:
 * iago_mcts_search_park's, explore_turns > 0: iago_mcts_search_explore's).  Refused (IAGO_ERR_INVALID): null args, n_fast
 * outside 1 .. n_sims, full_per_256 outside 1 .. 256, reserved fields not 0, an explore_turns outside 0 ..
 * IAGO_MAX_TURNS, a bad `park`, max_turns == 0, and match codes (2 / 3) in `active` (read as iago_mcts_search_park reads
 * it; not in a stream).  The wave search, matches and the arena do not cap.
 */
IAGO_API int iago_mcts_search_cap(const iago_mcts_search_args *args, const iago_search_cap_args *cap, void *stream);

/*
 * The rule above for the turn loop, one thread per game: fast[i] = 1 where turn[i] of the game with GLOBAL id game_id[i]
 * (id_base + G, as its 32 bits) is a fast turn under `seed` (the rollout seed; the XOR is applied here), else 0.
 * Refused (IAGO_ERR_INVALID): n < 0, a null array with n > 0, full_per_256 outside 1 .. 256.
 */
IAGO_API int iago_mcts_cap_mask(uint64_t seed, const int32_t *game_id, const int32_t *turn, int32_t full_per_256, int64_t n,
                                uint8_t *fast, void *stream);

/* ------------------------------------------------------------------ root noise */

#define IAGO_NOISE_KEY 0x44495249u /* ("DIRI") the urn's Philox key: the rollout seed with its high word XOR this */

typedef struct iago_root_noise {
    int32_t alpha_256; /* 1 .. 4096: alpha = alpha_256 / 256, the mass every legal cell starts with */
    int32_t eps_256;   /* 0 .. 256: eps = eps_256 / 256, the noise's share of a mixed prior */
    int32_t draws;     /* N: a power of two in 16 .. 1024, the urn's draws */
    int32_t reserved0; /* 0 */
    uint16_t *counts;  /* [n_games][64] the urn's counts by cell, one row per SLOT (tree) */
} iago_root_noise;

/*
 * ROOT NOISE in self-play, Dirichlet-style and in integers: at a searched turn t (the game's turn counter, passes
 * included) of the game with global id G, the priors of the root's children are mixed with the shares of a Polya urn.  Let
 * the mover have K legal moves, their cells in ascending order.
 *   - K < 2: nothing happens.  The counts are 0 and the single child, or the pass child, keeps its 1.1.
 *   - K >= 2, the urn: c[a] = 0 on every legal cell.  For j = 0 .. N-1 the weight of legal cell a is alpha_256 + 256 c[a],
 *     so the total is W = K alpha_256 + 256 j; w_j is word j & 3 of Philox4x32-10 on the counter (rollout->id_base + G, t,
 *     j >> 2, 0) under the key rollout->seed with its high word XOR IAGO_NOISE_KEY (a key of its own: not the explore
 *     draw's, the cap's, a match's or the replay window's); r = (uint64(w_j) * W) >> 32; the drawn cell is the lowest legal
 *     a with sum_{b <= a} weight[b] > r, and its c grows by 1.  The counts sum to N and are Dirichlet-multinomial(N, alpha):
 *     the shares c / N have granularity 1 / N and tend to Dirichlet(alpha) as N grows.
 *   - the mix, on the child's STORED prior p (what Node.__init__ keeps: prior + 0.1, MCTS.py:19): p becomes
 *     fadd_rn(fmul_rn(p, keep), term) with keep = float32((256 - eps_256) / 256) and term = float32(eps_256 c[a]) *
 *     2^-(8 + log2 N), both exact in float32; the product and the sum are each rounded once.
 *   - when: the root's children carry mixed priors for the whole of turn t's search, and the mix is applied ONCE.  A root
 *     that has children at the turn's start (a reused subtree) has them rewritten before the first playout; a root that
 *     expands during the turn's search (a fresh root at playout n_thr, a reused one with fewer than n_thr visits) creates
 *     its children with the mixed priors.  Nothing is undone afterwards: the children of a root were created while it was
 *     not the root, all but the chosen child are abandoned after the move, and the root moves every turn, passes included.
 *
 * iago_mcts_root_noise is the rule's first half for the turn loop, a sibling of iago_mcts_draw_move and
 * iago_mcts_cap_mask: for every game with active[g] != 0 (active NULL: every game) it draws the urn of turn[g] of the
 * game with GLOBAL id game_id[g] (id_base + G, as its 32 bits) over the legal moves of the mover of (root_own[g],
 * root_opp[g]) under `seed` (the rollout seed; the XOR is applied here), writes the counts row noise->counts[g][0 .. 63]
 * (0 off the legal set) and applies the mix to the children the tree's root already has.  Inactive games' rows and trees
 * are not touched.  Refused (IAGO_ERR_INVALID, nothing launched): a bad tree, a null array, alpha_256 outside 1 .. 4096,
 * eps_256 outside 0 .. 256, draws not a power of two in 16 .. 1024, a null counts buffer, reserved0 not 0.
 */
IAGO_API int iago_mcts_root_noise(const iago_mcts_tree *tree, const uint8_t *active, const uint64_t *root_own,
                                  const uint64_t *root_opp, uint64_t seed, const int32_t *game_id, const int32_t *turn,
                                  const iago_root_noise *noise, void *stream);

typedef struct iago_search_noise_args {
    iago_root_noise noise;        /* eps_256, draws and the counts buffer iago_mcts_root_noise filled (alpha_256 as there) */
    iago_search_streams *streams; /* optional: the role split of iago_mcts_search_split; NULL = the single launch */
    int64_t reserved[4];          /* 0 */
} iago_search_noise_args;

/*
 * The rule's second half: ONE search of iago_mcts_search_persistent (max_turns == 0; with `streams`
 * iago_mcts_search_split's) in which the tree root of every active game, where it expands in this search, creates its K
 * >= 2 children with the mixed priors of the game's row of noise.counts -- what iago_mcts_root_noise left there for this
 * turn.  Everything else -- the playouts, the rollouts' Philox streams, z_log, the totals -- is iago_mcts_search_persistent's;
 * with eps_256 = 0 the trees are, bit for bit.  `active` is a mask here (!= 0: searched).
 * Whole games (max_turns > 0, a stream) are NOT available: self-play with root noise runs turn by turn
 * (SelfPlayEngine's turn loop: iago_mcts_root_noise, then this search, per turn).  Under a playout cap the turn loop gives
 * the noise to the FULL games' search only (KataGo's rule): a fast turn searches the clean priors, so a fast turn is then
 * no longer a prefix of the full turn's search, as it is without noise.
 * Refused (IAGO_ERR_INVALID, nothing launched): null args, what iago_mcts_root_noise refuses of `noise`, reserved fields not
 * 0, max_turns > 0 or games_total > 0.  The wave search, matches and the arena do not noise.
 */
IAGO_API int iago_mcts_search_noise(const iago_mcts_search_args *args, const iago_search_noise_args *noise, void *stream);

/* ------------------------------------------------------------------ forced playouts and policy-target pruning */

/*
 * FORCED PLAYOUTS at the root of a noised search, and the pruning that takes them out of the policy target again (KataGo's
 * two rules), in exact arithmetic.  k_256 is an integer in 1 .. 4096, k = k_256 / 256 (KataGo's k = 2 is 512).
 *   forced(n, p, N):  n >= 1  and  float64(256 n n) < (float64(k_256) * float64(p)) * float64(N)
 * with n a child's visits, p its STORED float32 prior (after the + 0.1 of Node.__init__ and after the turn's noise mix) and
 * N the root's n_visits, the number whose square root Node.select takes.  The left side and the first product are exact in
 * float64, the second product rounds once; no contraction.  It says n < sqrt(k p N) without the root.
 *   - selection: in Node.select at the ROOT OF THE SEARCH only (the path's first node), when the root has K >= 2 children, a
 *     child with forced(n, p, N) scores +inf instead of Q + u; every other child scores as ever and the argmax is the first
 *     maximum, so the lowest-indexed forced child is taken.  Nothing changes below the root.  A reused root carries its N
 *     and its children's n from the turn before: the rule reads them as they are.
 *   - pruning, after the turn's search, for a root with K >= 2 children: b is the first child with the most visits
 *     (iago_mcts_best_move's), sq = sqrt(float64(N)), S* = Q_b + u_b as Node.select scores b under sq.  For every other
 *     child c with n >= 1 visits: F is the number of j in 1 .. n - 1 with forced(j, p_c, N); m = n; while n - m < F and the
 *     score of c with m - 1 visits (its Q and p as they are) is below S*, m -= 1; then, if m < n and m == 1, m = 0.  The
 *     pruned row has m at c's cell, n_b at b's, 0 off the children.  A root with fewer than two children keeps its raw row.
 *     The MOVE is still chosen from the raw counts (iago_mcts_best_move, iago_mcts_draw_move): only the target changes.
 *
 * iago_mcts_search_forced is iago_mcts_search_noise -- the same ONE search per launch, the same counts rows of
 * iago_mcts_root_noise, the single launch or with `streams` the role split -- with the selection rule above at every
 * active game's root.  Forcing lives only where the root noise lives: eps_256 = 0 forces without mixing.  The whole-game
 * launch, streams, the wave search, matches, the arena and the per-playout kernels do not force.
 * Refused (IAGO_ERR_INVALID, nothing launched): what iago_mcts_search_noise refuses (null args, a bad `noise`, reserved
 * fields not 0, max_turns > 0 or games_total > 0), k_256 outside 1 .. 4096.
 */
typedef struct iago_search_forced_args {
    iago_root_noise noise;        /* as iago_search_noise_args.noise */
    iago_search_streams *streams; /* optional: the role split of iago_mcts_search_split; NULL = the single launch */
    int32_t k_256;                /* 1 .. 4096: k = k_256 / 256 */
    int32_t reserved0;            /* 0 */
    int64_t reserved[4];          /* 0 */
} iago_search_forced_args;

IAGO_API int iago_mcts_search_forced(const iago_mcts_search_args *args, const iago_search_forced_args *forced, void *stream);

/*
 * The pruning rule above on the trees as they stand, a sibling of iago_mcts_best_move: for every game with active[g] != 0
 * (active NULL: every game) the pruned visit row of the tree's root into pruned[g][0 .. 63] -- for a root with fewer than
 * two children the raw row iago_mcts_best_move gives (0 everywhere for a root without children or with a pass child).
 * c_puct: the search's.  The trees are only read; inactive games' rows are not touched.
 * Refused (IAGO_ERR_INVALID, nothing launched): a bad tree, k_256 outside 1 .. 4096, null `pruned`.
 */
IAGO_API int iago_mcts_prune_visits(const iago_mcts_tree *tree, const uint8_t *active, float c_puct, int32_t k_256,
                                    int32_t *pruned /* [n_games][64] */, void *stream);

/*
 * iago_mcts_prune_visits under a selection rule: flags = 0 is that entry point exactly; flags = IAGO_SEARCH_PUCT_AZ scores
 * S* and every "score of c with m - 1 visits" with the AlphaZero rule's denominator, 1.0 + n (the trees of a search under
 * IAGO_SEARCH_PUCT_AZ).  forced() reads the stored priors as they are under both.
 * Refused (IAGO_ERR_INVALID, nothing launched): any other bit of flags, and what iago_mcts_prune_visits refuses.
 */
IAGO_API int iago_mcts_prune_visits_rule(const iago_mcts_tree *tree, const uint8_t *active, float c_puct, int32_t k_256,
                                         int32_t flags, int32_t *pruned /* [n_games][64] */, void *stream);

/*
 * The root's value, read back after a search -- a sibling of iago_mcts_best_move for the Value net's targets
 * (iago_value_targets, iago_hip_training.h).  For every game with active[g] != 0:
 *   n[g]   = the root's n_visits,
 *   q16[g] = the root's value for the root's MOVER in Q16.  Under IAGO_SEARCH_NEGAMAX a node's Q is the value for the
 *            player who moved INTO it, so the mover's value is -root.q (exact), and
 *              q16 = rint(-q * 65536):  one float32 multiply (by 2^16: exact), the conversion to nearest, ties to even,
 *            saturated to +-2^30 (a result beyond them is stored as the nearer one and raises bit 0 of *flags); a NaN q
 *            gives 0 and raises bit 1.  The Value net has no tanh, so |q| may exceed 1: nothing else is clipped here.
 * Games with active[g] == 0 get 0 and 0 (so does a root index outside the pool, which is not read).  One thread per game;
 * (n_visits, q) is the one 8-byte load Node.update takes.  The trees are only read.  Under the reference's backup rule a
 * root's Q mixes both players' views and is no value: the entry point cannot tell, its callers must (BatchedMCTS.root_value
 * refuses such an engine).  flags: optional, one word, or-ed into; the caller clears it.
 * Refused (IAGO_ERR_INVALID, before any device is touched): a NULL or bad tree, NULL active, q16 or n, n_games <= 0.
 */
#define IAGO_ROOT_VALUE_SATURATED 1
#define IAGO_ROOT_VALUE_NAN 2
IAGO_API int iago_mcts_root_value(const iago_mcts_tree *tree, const uint8_t *active, int32_t *q16 /* [n_games] */,
                                  int32_t *n /* [n_games] */, uint32_t *flags, void *stream);

/* ------------------------------------------------------------------ Gumbel root search */

#define IAGO_GUMBEL_KEY 0x47554D42u /* ("GUMB") the draw's Philox key: the rollout seed with its high word XOR this */

/*
 * THE GUMBEL ROOT SEARCH (Danihelka et al. 2022, "Policy improvement by planning with Gumbel"): at the root of a searched
 * turn m moves are sampled without replacement by Gumbel-top-k, the budget is spent on them by sequential halving, the
 * survivor is played, and the policy target is softmax(logit + sigma(completed Q)) instead of the visit counts.  Everything
 * that decides a move is in integers (Q16: units of 2^-16).
 *   - preconditions: the negamax backup (IAGO_SEARCH_NEGAMAX: a root child's Q is the root mover's value), the AlphaZero
 *     selection (IAGO_SEARCH_PUCT_AZ: a child's stored prior is the policy's p), ONE search per launch (max_turns 0,
 *     games_total 0), n_sims in 1 .. 32767, and a FRESH root (n_nodes == 1) in every searched game -- the caller resets the
 *     trees (BatchedMCTS.search does), so there is no subtree reuse under this rule.
 *   - two tables, computed by the caller in float64 and read by the device as they are (it calls neither log nor exp):
 *       gumbel_q16[u] = round(65536 * -ln(-ln((u + 0.5) / 65536))),  u = 0 .. 65535   (int32)
 *       ln_q16[i]     = round(65536 * ln(1 + (i + 0.5) / 4096)),      i = 0 .. 4095    (int32)
 *   - the draw (iago_mcts_gumbel_draw), before the search since it does not read the priors: for every active game g and
 *     every cell a, g[g][a] = gumbel_q16[c0 >> 16] with c0 word 0 of Philox4x32-10 on the counter (game_id[g], turn[g], a, 0)
 *     under the key `seed` with its high word XOR IAGO_GUMBEL_KEY (a key of its own).
 *   - the logit of a stored float32 prior p > 0 with biased exponent e and 23-bit mantissa f:
 *       logit_q16(p) = (e - 127) * 45426 + ln_q16[f >> 11]          (45426 = round(65536 ln 2); p == 1.0 likewise)
 *   - the schedule sched[k][i], int16 [m + 1][n_sims], built by the caller: row k lists, playout by playout, the visit count
 *     the next considered move must have when k moves are considered.  Rows 0 and 1 count 0, 1, 2, ...  For k >= 2 keep k
 *     counters at 0, L = ceil(log2 k), cur = k, and until the row is full: extra = max(1, n_sims / (L cur)) (integer
 *     division); extra times write the first cur counters and then add one to each of them; cur = max(2, cur / 2).  The row
 *     is cut at n_sims entries.  (k = 4, n_sims = 16: 0 0 0 0 1 1 1 1 2 2 3 3 4 4 5 5.)
 *   - selection, at the path's first node when it has K >= 2 children; every other node scores as ever.  t = the sum of the
 *     children's visits, maxN their largest, want = sched[min(m, K)][min(t, n_sims - 1)].  A child with n != want scores
 *     -inf; a child with n == want scores
 *       g[action] + logit_q16(p) + sigma,   sigma = ((c_visit + maxN) * c_scale_256 * q16) >> 8   (int64)
 *       q16 = (int)rintf(Q * 32768.0f) + 32768 for n > 0, 0 for n == 0 (the candidates are then all unvisited: it cancels)
 *     a sum below 2^53, carried as a float64; the first maximum wins (the lowest child index).  Stated on the visit counts
 *     alone, the rule keeps no state: the unvisited phase takes the top min(m, K) moves by g + logit, each later phase the
 *     better half of the phase before.  If NO child has n == want the children of the largest visit count are scored
 *     instead: this happens only where the preconditions were bypassed (a root that was not fresh).
 *   - the move and the rows (iago_mcts_gumbel_finish): of the children with the largest visit count the argmax of the same
 *     score, the lowest index on a tie; a root with one child (an only move, a pass: -1) or none (-2) answers as
 *     iago_mcts_best_move does.  Per game three rows [64] by cell: n (int32 visits), q (float32, 0 where unvisited) and
 *     logit (int32 logit_q16 of the stored prior; INT32_MIN off the root's children) -- what the improved-policy target is
 *     made from on the host (engine.gumbel_targets).
 */
typedef struct iago_gumbel_root {
    const int32_t *gumbel_q16; /* [65536] (the draw reads it) */
    const int32_t *ln_q16;     /* [4096] (the search and the finish read it) */
    const int16_t *sched;      /* [m + 1][n_sims] (the search reads it) */
    int32_t *g;                /* [n_games][64] the draws by cell, one row per SLOT (tree) */
    int32_t m;                 /* 2 .. 64: the moves considered */
    int32_t c_scale_256;       /* 1 .. 4096 (256: the paper's c_scale = 1) */
    int32_t c_visit;           /* 0 .. 4096 (50: the paper's) */
    int32_t reserved0;         /* 0 */
} iago_gumbel_root;

/*
 * The draw for the turn loop, a sibling of iago_mcts_root_noise: rows gumbel->g[g][0 .. 63] of every game with active[g] != 0
 * (active NULL: every game) at turn[g] of the game with GLOBAL id game_id[g]; inactive games' rows are not touched.  Reads
 * gumbel->gumbel_q16 and writes gumbel->g, nothing else.  Refused (IAGO_ERR_INVALID, nothing launched): a bad tree, a null
 * array, a null table or g, m / c_scale_256 / c_visit out of range, reserved0 not 0.
 */
IAGO_API int iago_mcts_gumbel_draw(const iago_mcts_tree *tree, const uint8_t *active, uint64_t seed, const int32_t *game_id,
                                   const int32_t *turn, const iago_gumbel_root *gumbel, void *stream);

typedef struct iago_search_gumbel_args {
    iago_gumbel_root gumbel;      /* the tables, the schedule of (m, args->n_sims), the rows iago_mcts_gumbel_draw filled */
    iago_search_streams *streams; /* optional: the role split of iago_mcts_search_split; NULL = the single launch */
    int64_t reserved[4];          /* 0 */
} iago_search_gumbel_args;

/*
 * ONE search of iago_mcts_search_persistent (max_turns == 0; with `streams` iago_mcts_search_split's) with the selection
 * rule above at every active game's root.  Everything else -- the playouts below the root, the rollouts' Philox streams,
 * z_log, the totals -- is iago_mcts_search_persistent's.  Whole games, streams of games, the wave search and the arena do
 * not take the rule: such games run turn by turn (draw, search, finish).
 * Refused (IAGO_ERR_INVALID, nothing launched, before the device is touched): null args, a null table / sched / g, m outside
 * 2 .. 64, c_scale_256 outside 1 .. 4096, c_visit outside 0 .. 4096, reserved fields not 0, max_turns > 0 or games_total >
 * 0, n_sims outside 1 .. 32767, games_per_workgroup without IAGO_SEARCH_NEGAMAX or without IAGO_SEARCH_PUCT_AZ.
 */
IAGO_API int iago_mcts_search_gumbel(const iago_mcts_search_args *args, const iago_search_gumbel_args *gumbel, void *stream);

/*
 * The move and the three rows of the rule above from the trees as they stand, a sibling of iago_mcts_best_move: for every
 * game with active[g] != 0 (active NULL: every game) move[g] and the rows n[g], q[g], logit[g] ([n_games][64] each).  Reads
 * gumbel->ln_q16, gumbel->g, c_scale_256 and c_visit; the trees are only read; inactive games are not touched.
 * Refused (IAGO_ERR_INVALID, nothing launched): a bad tree, a null array, what iago_mcts_gumbel_draw refuses of `gumbel`.
 */
IAGO_API int iago_mcts_gumbel_finish(const iago_mcts_tree *tree, const uint8_t *active, const iago_gumbel_root *gumbel,
                                     int8_t *move, int32_t *n, float *q, int32_t *logit, void *stream);

/* ------------------------------------------------------------------ arena */

/*
 * TWO searches of iago_mcts_search_persistent in ONE launch, each with its own nets: agent A (`a`) and agent B (`b`) are
 * complete argument sets of today's kind -- tree pool, roots and `active`, value / policy / rollout arguments, c_puct,
 * lmbda, n_thr, n_sims, cur_*, path, done, roll, leaf_value, rings (q_slots, ctl, rep_v / rep_p), totals, wg_own /
 * wg_opp, optional position table -- that share nothing but the grid and the clock.  Each agent's trees, moves, draws
 * and totals[0..1] are those of iago_mcts_search_persistent(a) / (b) run alone, bit for bit.
 *   - The grid: A's game workgroups, then B's, then the net workgroups -- the larger net_workgroups of the two sets
 *     (>= 2), cut to what is resident beside the games (the smaller positive max_cus of the two counts).
 *   - A net workgroup's HOME agent is the parity of its block index (even: A, odd: B; workgroup i runs on XCD i mod 8,
 *     so an XCD's L2 holds one agent's weights), its home ring inside that agent as in the single search.  It serves its
 *     home agent until that search is over -- every game workgroup of the agent has finished, or the agent gave up, or
 *     the clock limit passed -- then the other agent's; a game workgroup whose games are done does the same, its own
 *     agent first.
 *   - Every workgroup of the grid may walk either agent's nets: EACH agent's value->n and policy->n is at least
 *     4 x (both agents' game workgroups + the net workgroups) rows of its own wg_own / wg_opp.
 *   - The clock limit is the larger time_limit_ms.  An agent that gives up says so in ITS ctl[3]; the other one finishes.
 * Refused (IAGO_ERR_INVALID, nothing launched): a null set; whole games or a stream (max_turns > 0, games_total > 0:
 * the two trees of an arena game live in different workgroups); match codes (2 / 3) in an `active` (read back on
 * `stream` when device memory); two sets that share a tree, ctl, q_slots, reply or state arrays, wg_own / wg_opp or a
 * position table; net_workgroups < 2 in both; whatever iago_mcts_search_persistent refuses in either set.
 * IAGO_ERR_CAPACITY: both agents' game workgroups and two net workgroups do not fit the device together.  The wave
 * search, the role split, the hand-over and the exploring draw are not available here.
 */
IAGO_API int iago_mcts_search_arena(const iago_mcts_search_args *a, const iago_mcts_search_args *b, void *stream);

/* ------------------------------------------------------------------ a fixed-depth alpha-beta opponent */

#define IAGO_ALPHABETA_MAX_DEPTH 10
#define IAGO_OPENING_KEY 0x4F50454Eu /* ("OPEN") the opening draws' Philox key: the seed with its high word XOR this */

typedef struct iago_alphabeta_args {
    const uint64_t *own; /* [n] side to move (bit a = row*8+col) */
    const uint64_t *opp; /* [n] its opponent */
    int64_t n;
    int32_t depth;         /* 1 .. IAGO_ALPHABETA_MAX_DEPTH, one value per launch */
    int32_t time_limit_ms; /* 1 .. IAGO_ENDGAME_MAX_TIME_MS: the launch gives up after this long on the device clock */
    int16_t *score;        /* [n] out */
    int8_t *move;          /* [n] out */
    int64_t *nodes;        /* [n] out: nodes visited, leaves included */
    uint8_t *done;         /* [n] out: 1 = score and move are the search's */
    uint32_t *ctl;         /* [IAGO_ENDGAME_CTL_WORDS] cleared by the call; [0] != 0: gave up, [1]: the claim counter,
                              [2]: positions refused, [3] != 0: a stack overflow */
    int64_t reserved[4];   /* 0 */
} iago_alphabeta_args;

/*
 * A fixed-depth negamax search on a hand-written evaluation for n positions, one lane per position: an opponent that
 * owes nothing to the nets.  The rule, in integers, on the library's rules (a side with no legal move passes, the game
 * ends when neither side can move):
 *   search(own, opp, d):
 *       no legal move: neither side has one -> terminal(own, opp), at any depth; else -search(opp, own, d) (a pass in
 *       place: it costs no depth);
 *       d == 0 -> eval(own, opp);
 *       else the maximum over the legal moves m of -search(play(own, opp, m), d - 1).
 *   terminal = 10000 sign(D) + 100 D, D = #own - #opp (empty squares to nobody), so |terminal| <= 16400;
 *   eval = sum_k v_k (popcount(own & M_k) - popcount(opp & M_k)) + 8 (popcount(legal(own, opp)) - popcount(legal(opp, own)))
 *   over the seven classes (v, M) that partition the board and are invariant under its eight symmetries:
 *       100 0x8100000000000081   -20 0x4281000000008142   -50 0x0042000000004200   10 0x2400810000810024
 *         5 0x1800008181000018    -2 0x003C424242423C00    -1 0x00003C3C3C3C0000
 *   |eval| < 10000: any decided game outranks any heuristic; every value fits an int16 (the root's window is +-32767).
 * score[i] = search(own, opp, depth); move[i] = the LOWEST-indexed move whose value equals it -- found with
 * iago_solve_endgame's root rule, so (score, move) depend on neither move order nor pruning; -1: the mover must pass
 * (score is the negated value for the opponent), -2: the game is over.  nodes[i] counts the nodes visited.
 * A position with own & opp != 0 is refused: done[i] = 0, ctl[2] counts it.  done[] and ctl are cleared on `stream`
 * before the launch; it stops on its own clock after time_limit_ms (ctl[0] != 0, the unfinished positions keep
 * done[i] = 0).  Host-side refusals (IAGO_ERR_INVALID, nothing launched): a null args / ctl, a null array with n > 0,
 * n < 0, a depth or time_limit_ms out of range, reserved fields not 0.
 */
IAGO_API int iago_alphabeta_moves(const iago_alphabeta_args *args, void *stream);

#define IAGO_ALPHABETA_MAX_SPLIT 2
#define IAGO_ALPHABETA_SPLIT_CTL_WORDS 8

typedef struct iago_alphabeta_split_args {
    const uint64_t *own; /* [n] side to move */
    const uint64_t *opp; /* [n] its opponent */
    int64_t n;           /* at most 2^31 - 1 */
    int32_t depth;         /* 2 .. IAGO_ALPHABETA_MAX_DEPTH */
    int32_t split;         /* 1 .. IAGO_ALPHABETA_MAX_SPLIT, and at most depth - 1: the plies expanded into jobs */
    int32_t time_limit_ms; /* 1 .. IAGO_ENDGAME_MAX_TIME_MS, of the search stage */
    int32_t reserved0;     /* 0 */
    int16_t *score;        /* [n] out */
    int8_t *move;          /* [n] out */
    int64_t *nodes;        /* [n] out */
    uint8_t *done;         /* [n] out: 1 = every job of the root finished, score and move are the search's */
    int32_t *job_count;    /* [n] out: the jobs of root i */
    int64_t *job_first;    /* [n] out: the index of its first job (the exclusive sum of job_count) */
    int64_t job_capacity;  /* the jobs the arrays below hold, at most 2^31 - 1 */
    uint64_t *job_own;     /* [job_capacity] out: the job's side to move */
    uint64_t *job_opp;     /* [job_capacity] out */
    int32_t *job_root;     /* [job_capacity] out: the root it belongs to */
    int8_t *job_path;      /* [job_capacity][4] out: depth left, first move, second move (-1 where absent), 0 */
    int16_t *job_score;    /* [job_capacity] out: search(job_own, job_opp, depth left) */
    int8_t *job_move;      /* [job_capacity] out */
    int64_t *job_nodes;    /* [job_capacity] out */
    uint8_t *job_done;     /* [job_capacity] out */
    uint32_t *ctl;         /* [IAGO_ALPHABETA_SPLIT_CTL_WORDS] cleared by the call; [0] != 0: gave up, [1]: the claim
                              counter, [2]: positions refused, [3] != 0: a stack overflow, [4] / [5]: the low / high word
                              of the jobs needed, [6] != 0: they exceed job_capacity (nothing was searched), [7]: 0 */
    int64_t reserved[4];   /* 0 */
} iago_alphabeta_split_args;

/*
 * iago_alphabeta_moves with every root's search spread over many lanes: the same (score, move) for every position, bit
 * for bit, from one call on `stream` with no host round trip inside it.  The rule, in integers: a node (own, opp) with d
 * depth left and k split plies left (the root: depth, split)
 *   - is a JOB (own, opp, d) when k == 0 or its mover has no legal move: its value is search(own, opp, d) from its
 *     mover's view, what iago_alphabeta_moves returns for that position at depth d, found with the full window, and its
 *     nodes are that call's;
 *   - is EXPANDED otherwise: its children are its legal moves in ascending index, each with (d - 1, k - 1), its value
 *     the maximum of the negated children's values.
 * So a root that must pass or whose game is over is one job of the full depth and its move is the job's (-1 / -2); a
 * child that cannot move is one job of depth - 1; every other job has depth - split >= 1 left.  move[i] is the
 * lowest-indexed move whose value equals score[i]; nodes[i] = the nodes expanded (the root, and at split 2 every
 * expanded child) + the sum of its jobs' nodes, so it depends on no timing.
 * Three stages: (1) the jobs of every root are counted (job_count), summed (job_first; ctl[4] / [5] = their total) and
 * written in canonical order -- root ascending, then first move, then second move; (2) the lanes of
 * iago_alphabeta_moves' search claim jobs one at a time, each with its own depth; (3) a thread per root takes its run of
 * jobs back, the sign turned once per ply of the path.  More jobs than job_capacity: ctl[6] is set, nothing is
 * searched, every done[i] stays 0 and nothing is written past the capacity.  The COUNT-ONLY form -- every job_* array
 * null and job_capacity 0 -- writes job_count, job_first and ctl[4] / [5] and launches nothing else (score, move, nodes
 * and done may be null then; ctl[6] stays 0).  A position with own & opp != 0 is refused as there: ctl[2] counts it, it
 * has no job and done[i] = 0.  The give-up is the search stage's, as there: ctl[0] != 0, done[i] = 0 for every root with
 * an unfinished job.  Host-side refusals (IAGO_ERR_INVALID, nothing launched): a null args / ctl / own / opp /
 * job_count / job_first with n > 0, n < 0 or above 2^31 - 1, a depth above IAGO_ALPHABETA_MAX_DEPTH, a split outside
 * 1 .. IAGO_ALPHABETA_MAX_SPLIT or not below depth, a time_limit_ms out of range, a job_capacity below 0 or above
 * 2^31 - 1, some but not all job_* arrays null or null ones with a capacity, a null score / move / nodes / done outside
 * the count-only form, reserved fields not 0.
 */
IAGO_API int iago_alphabeta_moves_split(const iago_alphabeta_split_args *args, void *stream);

/*
 * The random opening of a match against that opponent, a thread per game: the mover of game g (own[g] to move) with
 * K >= 1 legal moves plays the r-th lowest legal cell, r = (uint64(w) * K) >> 32, w = word turn & 3 of Philox4x32-10 on
 * the counter (id_base + g mod id_mod, turn >> 2, 0, 0) under the key `seed` with its high word XOR IAGO_OPENING_KEY (the
 * raw word, no float).  move[g] = -1 where the mover has no legal move.  id_mod = n / 2 gives games g and g + n / 2 the
 * same draws (a paired match), id_mod = n every game its own.  Refused (IAGO_ERR_INVALID): a null array with n > 0,
 * n < 0, id_mod == 0, a turn outside 0 .. IAGO_MAX_TURNS - 1.
 */
IAGO_API int iago_random_moves(const uint64_t *own, const uint64_t *opp, int64_t n, uint64_t seed, uint32_t id_base,
                               uint32_t id_mod, int32_t turn, int8_t *move, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* IAGO_HIP_SERVING_H */
