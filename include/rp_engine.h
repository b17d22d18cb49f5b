/*
 * rp_engine.h -- C ABI of the MI355X-native self-play bin-packing engine
 * (librp_engine.so, built from resource_packing_self_play_amd/csrc/rp_engine.hip).
 *
 * The reference (Wang-Xiaoyang/resource_packing_self_play) is pure Python and has
 * no FFI; its boundary for this path is the duck-typed plugin API that
 * xw_mcts/main_bpp.py:93-121 and xw_mcts/CoachBPP.py drive.  Each entry point
 * below names the reference method(s) it replaces (paths relative to
 * /root/reference/xw_mcts).  The Python classes with the reference's names
 * (resource_packing_self_play_amd.{binpacking.BinPackingGame, MCTS_bpp, CoachBPP,
 * binpacking.pytorch.NNet}) are thin ctypes callers of this ABI; INTEGRATION.md
 * shows the binding a reference maintainer would add.
 *
 * Conventions
 *   - plain C types only; no torch / HIP types in signatures (streams and device
 *     buffers cross as void* / raw device pointers).
 *   - every function returns 0 on success or a negative rp_status; the message is
 *     available from rp_last_error().  No exception crosses the ABI.
 *   - the caller owns every buffer it passes; the library owns everything reachable
 *     from rp_ctx.  Inputs are never modified unless documented as in/out.
 *   - one rp_ctx per (process, GPU), externally synchronised; all device work is
 *     enqueued on the stream given at create time.
 *   - a state is (rows, remaining): rows[r] is the W-bit occupancy of grid row r
 *     (bit c = cell (r, c)), always passed as uint64; remaining[i] != 0 iff item i is
 *     still unplaced; item sizes are (w, h) bytes.  action = item * W + column, as
 *     BinPackingGame.py:67,91.
 *   - limits: 1 <= W <= 64, 1 <= H <= 64, 1 <= N <= 128.
 */
#ifndef RP_ENGINE_H
#define RP_ENGINE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define RP_ABI_VERSION 10  /* 4: sparse replay buffer (rp_config.max_sparse, rp_examples_packed*, rp_expand_examples), rp_leaf_count_async
                             5: placement trace (rp_set_trace, rp_pop_finished_packings)
                             6: softmax in the commit kernel for every action space (rp_commit_eval_logits_wide, rp_debug_commit_plan)
                             7: the commit kernel's softmax as a self-test (rp_selftest_softmax)
                             8: random-playout leaf evaluator (rp_rollout_eval, rp_rollout_states)
                             9: initial states of pool instances (rp_set_instance_initial)
                             10: incumbents (rp_set_incumbent, rp_pop_finished_best, rp_incumbents); additive, same number: playout
                                 incumbents (rp_set_incumbent_playouts, rp_pop_finished_best_playouts, rp_incumbent_sources, rp_rollout_paths), the
                                 playout policy (rp_set_playout_policy, rp_playout_policy), the rollout prior (rp_set_rollout_prior,
                                 rp_rollout_prior, rp_rollout_prior_states) and the playouts' landing power (rp_set_playout_landing,
                                 rp_playout_landing) */

typedef enum rp_status {
    RP_OK = 0,
    RP_ERR_ARG = -1,        /* bad argument */
    RP_ERR_DEVICE = -2,     /* HIP error (no GPU, launch failure, ...) */
    RP_ERR_CAPACITY = -3,   /* a per-game node / legal-move / visited-edge arena, the finished-episode ring or the replay buffer
                               overflowed: a device error, see "device errors" at rp_check */
    RP_ERR_ASSERT = -4,     /* a precondition the reference asserts was violated
                               (BinPackingGame.py:69 item already placed, :89 no legal move) */
    RP_ERR_STATE = -5       /* call not valid in the engine's current phase */
} rp_status;

/* how a finished search turns into a move (CoachBPP.py:86-87 draws from OS entropy,
 * which cannot be reproduced; the engine offers deterministic rules instead) */
typedef enum rp_move_rule {
    RP_MOVE_EXTERNAL = 0,   /* host supplies actions through rp_advance_roots */
    RP_MOVE_ARGMAX_FIRST = 1, /* lowest-index argmax of the root visit counts */
    RP_MOVE_SAMPLE = 2,     /* a ~ counts with a counter-based RNG keyed by (seed, episode id, move) */
    RP_MOVE_ARGMAX_DRAW = 3, /* argmax of the root visit counts, ties drawn uniformly (MCTS_bpp.py:45-46): entry umulhi(x, m) of the
                             * m most-visited actions in ascending order, x from the RP_MOVE_SAMPLE stream of (episode id, move) */
    RP_MOVE_INCUMBENT = 4   /* the move of CoachBPP.py:86-99 follows the episode's incumbent (rp_set_incumbent): keep the best line and play
                             * along it, the usual step of single-player Monte-Carlo search.  When a slot's search budget is spent, m moves
                             * have been played and I is its running incumbent -- what rp_incumbents would return at that moment, every
                             * offer of the move's simulations made (tree terminals, MCTS_bpp.py:78-83, and under rp_set_incumbent_playouts
                             * the playouts of MCTS_bpp.py:87).  I is FOLLOWABLE iff (1) the slot has one (moves >= 0), (2) score > 0 -- a
                             * score of 0 is a packing that dropped an item (getRankedReward, BinPackingGame.py:188-212); the first terminal
                             * of an episode enters the record even so, and such a line leads nowhere --, (3) I.moves > m: it has a next
                             * action, (4) I.action[q] == the move played at q for every q < m: its line passes through the root.  If I is
                             * followable the move is I.action[m], played exactly as rp_advance_roots plays an external action (getNextState,
                             * BinPackingGame.py:58-76): a legal move the search never tried gets its visited entry, a child that does not
                             * exist yet is materialised and, if terminal, offered.  Otherwise the move is RP_MOVE_ARGMAX_FIRST's.  Examples
                             * (the root's visit counts, or the one-hot on the played action), trace, the played prefix of the incumbent
                             * record and the restart are those of every rule.  Condition 4 makes the rule well defined after a mid-episode
                             * rp_set_move_rule and under every order of calls; with the rule in force since the episode began it always
                             * holds for an incumbent with score > 0, because a replacement is found from the current root.  Consequences:
                             *  - under the rule from the start of an episode, a finished episode with best score > 0 has best action ==
                             *    the played actions, best score == played score, best outcome == played outcome, best board == final board;
                             *  - the rule reads nothing but the incumbent record and the root, so the played line stays a function of the
                             *    search alone: not of the slot, rp_set_step_cap, rp_set_compact_rows or graph replay;
                             *  - counter [14] of rp_counters counts the moves that followed the incumbent; 0 under rules 0 to 3.
                             * Needs the incumbents: rp_set_move_rule(ctx, 4, ..) while they are off and rp_set_incumbent(ctx, 0) while the
                             * rule is in force are RP_ERR_STATE, rp_create with move_rule == 4 is RP_ERR_ARG (a new context keeps no
                             * incumbents yet: set the rule afterwards); a refused call changes nothing. */
} rp_move_rule;

/* game phases reported by rp_game_status; RP_PHASE_FAILED: a device error stopped this slot's episode (see rp_check) */
enum { RP_PHASE_IDLE = 0, RP_PHASE_RUNNING = 1, RP_PHASE_WAIT_EVAL = 2, RP_PHASE_MOVE_READY = 3,
       RP_PHASE_EPISODE_DONE = 4, RP_PHASE_FAILED = 5 };

/* kinds of a stored Q / backed-up value (NumPy promotion state):
 * 0 weak (Python int/float, f64 arithmetic), 1 float32, 2 strong float64 */
enum { RP_KIND_WEAK = 0, RP_KIND_F32 = 1, RP_KIND_F64 = 2 };

typedef struct rp_config {
    int32_t abi_version;   /* RP_ABI_VERSION */
    int32_t W, H, N;       /* BinPackingGame(bin_width, bin_height, num_items, n) BinPackingGame.py:15 */
    int32_t games;         /* concurrent game slots G on this GPU */
    int32_t sims;          /* args.numMCTSSims (MCTS_bpp.py:37) */
    double cpuct;          /* args.cpuct (MCTS_bpp.py:114,117); must be > 0 (see rp_commit_eval) */
    double alpha;          /* args.alpha (MCTS_bpp.py:79) */
    int32_t node_cap;      /* per-game node arena; 0 = sims * (N + 1) + 2 */
    int32_t edge_cap;      /* per-game legal-move arena (one 6-byte entry per legal move of every node); 0 = automatic */
    int32_t move_rule;     /* rp_move_rule */
    int32_t auto_restart;  /* 1: a finished slot pulls the next instance from the pool set by rp_set_instance_pool */
    int32_t reclaim;       /* 1: when a move is played, the arena chunks of the old root's level are recycled (its states
                              are unreachable from then on); do not re-root to shallower states afterwards */
    int32_t reserved0;
    uint64_t seed;         /* RNG seed for RP_MOVE_SAMPLE and the tie rule */
    uint64_t tie_salt;     /* salt of the deterministic stand-in for np.random.choice([1,-1]) (BinPackingGame.py:212) */
    int32_t device;        /* HIP device ordinal */
    int32_t vis_cap;       /* per-game visited-edge arena (32-byte entries); 0 = automatic */
    void *stream;          /* hipStream_t; NULL = the default stream */
    int64_t max_examples;  /* capacity of the replay buffer in examples; 0 = none recorded */
    int64_t max_sparse;    /* capacity of the replay buffer's pool of (action, visit count) pairs -- one per visited root edge of every
                              recorded example; 0 = automatic (max_examples x min(A, sims + 1, 64)) */
} rp_config;

typedef struct rp_ctx rp_ctx;

/* ---- life cycle ---------------------------------------------------------------------- */
int rp_version(void);
/* MCTS.__init__ (MCTS_bpp.py:16-26) + BinPackingGame.__init__ (BinPackingGame.py:15-22) for G games */
int rp_create(const rp_config *cfg, rp_ctx **out);
void rp_destroy(rp_ctx *ctx);
/* message of the last failing call on this ctx (or of rp_create when ctx == NULL) */
const char *rp_last_error(const rp_ctx *ctx);
/* bytes of HBM the ctx holds */
int64_t rp_device_bytes(const rp_ctx *ctx);

/* ---- stateless game rules over a batch of B states (host pointers) -------------------- */
/* BinPackingGame.getValidMoves (BinPackingGame.py:78-92) -> Bin.get_moves_for_square /
 * get_adjacency (BinPackingLogic.py:47-93).  mask_out[b][a] in {0,1}; n_valid_out may be NULL.
 * A state without a legal move yields an all-zero row (the shim raises the reference's
 * AssertionError of BinPackingGame.py:89). */
int rp_valid_moves(rp_ctx *ctx, int64_t B, const uint64_t *rows /*[B][H]*/, const uint8_t *remaining /*[B][N]*/,
                   const uint8_t *item_wh /*[B][N][2]*/, uint8_t *mask_out /*[B][W*N]*/, int32_t *n_valid_out /*[B]*/);
/* BinPackingGame.getNextState (BinPackingGame.py:58-76) -> Bin.execute_move (BinPackingLogic.py:95-109).
 * status_out[b] = 0, or RP_ERR_ASSERT when the item is already placed (BinPackingGame.py:69). */
int rp_apply_move(rp_ctx *ctx, int64_t B, const uint64_t *rows, const uint8_t *remaining, const uint8_t *item_wh,
                  const int32_t *action /*[B]*/, uint64_t *rows_out, uint8_t *remaining_out, int32_t *status_out);
/* BinPackingGame.getGameEnded (BinPackingGame.py:109-116) -> has_valid_moves (:94-107) and
 * getRankedReward (:188-212).  ended_out[b] = 0 (a move exists), +1, -1, or 2 for the r == bl
 * tie branch (the caller draws); reward_out[b] = r.  rewards is the R2 buffer shared by the batch. */
int rp_game_ended(rp_ctx *ctx, int64_t B, const uint64_t *rows, const uint8_t *remaining, const uint8_t *item_wh,
                  const int32_t *total_area /*[B]*/, const int32_t *max_h /*[B]*/, const double *rewards, int32_t n_rewards,
                  double alpha, int32_t *ended_out, double *reward_out);

/* ---- episode set-up ------------------------------------------------------------------ */
/* Items of game slot(s): BinPackingGame.getInitItems (BinPackingGame.py:37-51, also fixes max_h)
 * and CoachBPP.items_total_area (CoachBPP.py:34,119).  Starts a new episode for slots
 * first..first+count-1 at the empty board with an empty tree (CoachBPP.py:67-68,124). */
int rp_begin_episodes(rp_ctx *ctx, int32_t first, int32_t count, const uint8_t *item_wh /*[count][N][2]*/,
                      const int32_t *total_area /*[count]*/, const uint64_t *episode_id /*[count] or NULL*/);
/* Pool of instances for auto_restart: slot g takes instance g at rp_begin_pool and a finished
 * slot takes the next unused one; episode id = pool index + first_id. */
int rp_set_instance_pool(rp_ctx *ctx, int64_t n_instances, const uint8_t *item_wh /*[n][N][2]*/,
                         const int32_t *total_area /*[n]*/, uint64_t first_id);
int rp_begin_pool(rp_ctx *ctx);
/* ItemsGenerator.items_generator(seed) (BinPackingGame.py:257-285) on device: guillotine cuts of the bin_w x bin_h rectangle
 * into N items, bit-identical to the reference's NumPy stream (np.random.seed = MT19937 init_genrand, legacy randint = masked
 * rejection on 32-bit draws).  rp_generate_items returns the (w, h) pairs to the host; rp_set_instance_pool_seeds fills the
 * auto_restart pool directly on device (total area bin_w * bin_h as CoachBPP.py:119). */
int rp_generate_items(rp_ctx *ctx, int64_t n, const uint32_t *seeds /*[n]*/, int32_t bin_w, int32_t bin_h, uint8_t *item_wh_out /*[n][N][2]*/);
int rp_set_instance_pool_seeds(rp_ctx *ctx, int64_t n_instances, const uint32_t *seeds, int32_t bin_w, int32_t bin_h, uint64_t first_id);
/* Optional per-instance metadata of the pool set last by rp_set_instance_pool*: instance i plays as episode episode_id[i] (instead
 * of first_id + i) and is ranked against the R2 threshold (bl[i], has_buf[i]) (instead of the rp_set_rank_buffer snapshot).  Any
 * array may be NULL (that field keeps its default); n must equal the pool's size.  The next rp_set_instance_pool* clears it.  The
 * metadata lives in device memory, so captured graphs stay valid. */
int rp_set_instance_meta(rp_ctx *ctx, int64_t n, const uint64_t *episode_id /*[n]*/, const double *bl /*[n]*/, const uint8_t *has_buf /*[n]*/);
/* Optional initial state of every instance of the pool set last by rp_set_instance_pool*: instance i starts at
 * (rows[i], remaining[i]) instead of the empty bin with all N items (CoachBPP.py:67-68).  remaining[i][k] == 0: item k does not
 * take part (its plane is zero from the first state on, BinPackingGame.py:86); its item_wh bytes are ignored.  max_h NULL:
 * max_h[i] = largest h among the items with remaining != 0 (getInitItems, BinPackingGame.py:48, over the items that take part; 0
 * if none); otherwise the caller's value (continuing an episode whose placed items count).  total_area stays what the pool was
 * given: the caller includes the cells already set.  Moves are numbered from 0 at the initial state (sampling streams, trace,
 * examples).  An instance whose initial state has no legal move is an episode of 0 moves: outcome and score are getGameEnded of
 * that state (tie drawn as for Es), it gets a finished record (final bin = initial rows) and the slot takes the next instance.
 * n must equal the pool's size; a row with a bit at or above W -> RP_ERR_ARG.  rows and remaining both NULL clears it; the next
 * rp_set_instance_pool* clears it.  Device memory: captured graphs stay valid. */
int rp_set_instance_initial(rp_ctx *ctx, int64_t n, const uint64_t *rows /*[n][H]*/, const uint8_t *remaining /*[n][N]*/,
                            const int32_t *max_h /*[n] or NULL*/);
/* R2 buffer snapshot (rewards_list argument of MCTS.getActionProb / getGameEnded, CoachBPP.py:76-91):
 * the threshold sorted[int(floor(len*alpha))-1] is recomputed and used by every slot from now on. */
int rp_set_rank_buffer(rp_ctx *ctx, const double *rewards, int32_t n);
/* Re-root slot(s) at an arbitrary state without clearing the tree (MCTS.getActionProb called with a
 * new canonicalBoard on the same MCTS object, CoachBPP.py:74-78).  RP_ERR_STATE while incumbents are on (rp_set_incumbent): the engine
 * does not know the moves that lead to the new root, so it could not say how an incumbent found from there is reached. */
int rp_set_roots(rp_ctx *ctx, int32_t first, int32_t count, const uint64_t *rows /*[count][H]*/,
                 const uint8_t *remaining /*[count][N]*/);

/* Moves the context to another HIP stream (e.g. the side stream of a hipGraph capture: rp_search_step(ctx, NULL),
 * rp_leaf_planes and rp_commit_eval only enqueue work, so a whole simulation wave can be captured and replayed). */
int rp_set_stream(rp_ctx *ctx, void *stream);
/* Bounds the simulations one slot runs inside one rp_search_step (0 = unbounded, the default).  Slots near the end of a
 * game hit cached terminal states (Es, MCTS_bpp.py:81-83) and need no evaluator; the cap keeps such a slot from stretching
 * the launch for everyone.  Scheduling only -- results are identical for any value. */
int rp_set_step_cap(rp_ctx *ctx, int32_t max_sims_per_step);
/* Compact evaluator rows without a host round trip: with enable != 0, rp_search_step(ctx, NULL) also lists the waiting slots in
 * slot order on the device (row b = b-th waiting slot, as with a count request), rp_leaf_stem / rp_leaf_planes / rp_commit_eval
 * follow that list, and the rp_nn_resstage16 / rp_nn_resstage32 / rp_nn_convpool32 launches of this context stop at the number of
 * waiting leaves (read on the device), so slots that wait for nothing -- finished episodes, terminal streaks -- cost no
 * convolution work.  Rows past the count hold stale data.  Scheduling only: results do not depend on it. */
int rp_set_compact_rows(rp_ctx *ctx, int32_t enable);
/* Switches the move rule; onehot_examples != 0 records pi as a one-hot on the played action, the greedy branch of
 * MCTS.getActionProb (greedy_a == 0, MCTS_bpp.py:43-49) that CoachBPP uses after iterStepThreshold (CoachBPP.py:132).  RP_ERR_ARG outside
 * rp_move_rule; RP_ERR_STATE for RP_MOVE_INCUMBENT while incumbents are off.  A refused call changes nothing. */
int rp_set_move_rule(rp_ctx *ctx, int32_t move_rule, int32_t onehot_examples);
/* Placement trace: with enable != 0 every move played on the device -- by any rp_move_rule, rp_advance_roots included -- is recorded
 * as (action, rows): action = item * W + column as BinPackingGame.getNextState takes it (BinPackingGame.py:58-76, item and column
 * split at :67), rows = bit r set iff the move filled cells of bin row r.  Bin.execute_move (BinPackingLogic.py:95-109) fills the
 * first h free row segments scanning from row 0, so the rows of one move may be non-contiguous, and fewer than h where the strip
 * runs out; they are read off as the rows where the new root's key differs from the old one's, which costs the search nothing.
 * When an episode ends its moves and final bin -- what the reference's display(board) prints (BinPackingGame.py:232) -- are kept
 * next to its finished record for rp_pop_finished_packings.  Refused with RP_ERR_STATE while any slot is in the middle of an episode.
 * The buffers are allocated on the first enable: fin_cap * (10 N + 8 H) bytes for the ring (fin_cap = max(4 G, 1024)) plus 10 G N
 * for the running episodes -- 73 MB at 32 768 slots of 20x20 / 32 items in two contexts; with the trace off nothing is allocated and
 * the kernels take one uniform branch.  Kernel arguments are baked into captured graphs: re-capture after switching, as after
 * rp_set_move_rule.  Records of episodes that finished while the trace was off carry no trace: drain the ring before switching. */
int rp_set_trace(rp_ctx *ctx, int32_t enable);
/* Incumbents: with enable != 0 every episode of a slot carries the best complete packing its search saw.  The search fills Es once per
 * state, when it first meets it (MCTS_bpp.py:78-83), and a state without a legal move is scored there by getRankedReward
 * (BinPackingGame.py:188-212); the reference keeps the sign only.  The incumbent is defined over the terminal states MATERIALISED in the
 * slot's tree during the episode, in creation order -- by a simulation of rp_search_step, by a played move whose child did not exist
 * yet (any rp_move_rule, rp_advance_roots included), by the episode's initial state when it is terminal, by rp_begin_episodes: a new
 * terminal with score r replaces the incumbent iff r is strictly greater, and an episode starts without one, so the first terminal
 * always enters (even with r == 0) and the first created among equals stays.  The record: score (that r), outcome (the node's Es, the
 * r == bl tie resolved as the search resolves it), moves, action[moves] from the episode's initial state = the moves played so far
 * followed by the creating simulation's path, prefix (the number of played moves when it was found), board (the terminal's H row masks)
 * and updates (how often the incumbent was replaced in this episode, the first entry included).  Every finished episode has one -- its
 * own final state was materialised -- so best score >= played score always.  The record is a function of the search alone: not of
 * rp_set_step_cap, rp_set_compact_rows, the slot, or graph replay.  Playouts of rp_rollout_eval feed it only under
 * rp_set_incumbent_playouts (below); by default: tree terminals only.
 * Refused with RP_ERR_STATE while any slot is in the middle of an episode.  The buffers are allocated on the first enable:
 * (G + fin_cap) * S + 16 G bytes, S = 24 + 8 H + 4 N rounded up to a multiple of 8 and fin_cap = max(4 G, 1024) -- 52 MB at 32 768 slots
 * of 20x20 / 32 items in two contexts; with incumbents off nothing is allocated and every hook is one uniform branch.  While they are
 * on, rp_search_step launches one more small kernel, and a slot's launch ends with the simulation that brought a terminal into its tree
 * (it goes on in the next one, as under rp_set_step_cap: scheduling only).  Kernel arguments are baked into captured graphs: re-capture
 * after switching.  Records of episodes that finished while incumbents were off carry none: drain the ring before switching.
 * rp_set_roots is refused while they are on.  rp_set_incumbent(ctx, 0) is RP_ERR_STATE while RP_MOVE_INCUMBENT is in force. */
int rp_set_incumbent(rp_ctx *ctx, int32_t enable);
/* Playout incumbents: with enable != 0 every playout that rp_rollout_eval runs for a waiting leaf (MCTS_bpp.py:87) is a candidate for
 * the slot's incumbent too -- plain single-player MCTS practice: keep the best rollout.  Off by default; off, records, device bytes and
 * the playout kernel's path are what they are without this call.  The candidates of an episode form ONE sequence in simulation order.
 * Tree terminals enter it exactly as under rp_set_incumbent (a slot's launch ends at the simulation that materialised a terminal and
 * the offer is made behind it).  Each evaluated leaf enters it with one offer, at the place of the simulation that reached it: the
 * leaf's best playout -- the largest score r (getRankedReward, BinPackingGame.py:188-212, of the playout's final bin), the lowest
 * playout index j among equals.  An offer replaces the incumbent iff the slot has none yet or r is strictly greater, so `updates`
 * grows by at most one per leaf, and a second rp_rollout_eval for the same waiting leaves changes nothing.  The record of a playout
 * incumbent: score = r; outcome = the playout's resolved outcome (the r == bl tie drawn from its final state as for Es); board = the
 * playout's final rows; prefix = the number of moves played when it was found; action = the played moves, then the leaf's path (the
 * path rp_search_step stores for the commit), then the playout's own moves, each item * W + column as getNextState takes it
 * (BinPackingGame.py:58-76); moves = their total.  Two more fields say where a record came from: tree_moves = prefix + path length
 * (the leaf is reached after that many actions) and playout = j, or -1 for a tree terminal, for which tree_moves == moves.  The record
 * stays a function of the search alone: not of rp_set_step_cap, rp_set_compact_rows, the slot, graph replay or the evaluator row.  The
 * episode's own final state is still materialised in the tree, so best score >= played score still holds.
 * RP_ERR_STATE while incumbents are off and while any slot is in the middle of an episode; rp_set_incumbent(ctx, 0) turns this off too.
 * The two fields live in a side array of 8 (G + fin_cap) bytes allocated on the first enable; the records' stride S does not change.
 * Kernel arguments are baked into captured graphs: re-capture after switching. */
int rp_set_incumbent_playouts(rp_ctx *ctx, int32_t enable);
/* Changes args.numMCTSSims for the following searches (MCTS_bpp.py:37); rp_search_step stops a slot after this many
 * simulations from its current root. */
int rp_set_sims(rp_ctx *ctx, int32_t sims);

/* ---- search: MCTS.search (MCTS_bpp.py:56-139) in lock step over all slots ------------- */
/* Runs simulations for every RUNNING slot until each either needs a leaf evaluated (the
 * nnet.predict call of MCTS_bpp.py:87) or has finished its args.numMCTSSims budget
 * (select :106-121, descend :125-128, terminal :78-83, backup :130-139 on device).
 * Enqueues work only; *n_leaves_out (may be NULL) forces a stream sync and returns the number of
 * leaves waiting for evaluation. */
int rp_search_step(rp_ctx *ctx, int32_t *n_leaves_out);
/* Writes the evaluator input of the waiting leaves, FP32 NCHW [n][N+1][H][W] exactly as
 * BinPackingGame.getBinItem + NNet.predict's view (BinPackingGame.py:118-120, NNet.py:77-79),
 * into caller-owned DEVICE memory (capacity_rows rows). */
int rp_leaf_planes(rp_ctx *ctx, float *planes_dev, int64_t capacity_rows);
/* Measurement aid: enqueues a copy of the current number of waiting leaves (the device-side count of rp_set_compact_rows /
 * rp_search_step) into HOST memory (pinned, or the copy synchronises) without waiting for it. */
int rp_leaf_count_async(rp_ctx *ctx, int32_t *count_host);
/* Evaluator stem on device: the network's first convolution + max-pool (BinpackingNNet.py:34,39-40:
 * conv_seqs[0].conv 3x3 pad 1, N+1 -> 16 channels, then max_pool2d(3, stride 2, pad 1)) evaluated straight from the packed
 * leaf states, exploiting that item planes are origin-anchored rectangles (tabulated tap sums).  rp_stem_set_weights reads
 * the DEVICE weight [16][N+1][3][3] and bias [16] tensors and rebuilds the tables (call again after every weight update);
 * rp_leaf_stem writes FP32 [n][16][(H+1)/2][(W+1)/2] into caller-owned DEVICE memory, the input of conv_seqs[0].res_block0.
 * The tap sums are tabulated in per-channel fixed point (float64 sums quantised to int32, unit 2^-k chosen from the channel's
 * bound), added as integers and converted to float32 once: within (N + 2) half units + half an ulp of the exact sum, i.e. the
 * correctly rounded convolution for practical purposes; rp_leaf_planes + the two PyTorch ops differ from it by their own
 * float32 summation error. */
int rp_stem_set_weights(rp_ctx *ctx, const float *conv_w_dev, const float *bias_dev);
int rp_leaf_stem(rp_ctx *ctx, float *out_dev, float *out_relu_dev /* relu(out), may be NULL */, int64_t capacity_rows,
                 int32_t channels_last /* 0: [n][16][Hp][Wp], 1: [n][Hp][Wp][16] (MIOpen's FP32 kernels are faster on NHWC) */);
/* Fused element-wise pieces of the evaluator on the context's stream (NCHW float32 DEVICE tensors).  PyTorch-ROCm runs the
 * bias add of a convolution, each ReLU, the residual add and the max-pool of BinpackingNNet.py:21-27,39-40 as separate
 * HBM-bound kernels; these apply the same operations in the same order in one pass:
 *   rp_nn_bias_relu      x = relu(x + bias[c])                                       (in place)
 *   rp_nn_bias_residual  out = (x + bias[c]) + res ; out_relu = relu(out)            (out_relu may be NULL)
 *   rp_nn_bias_pool      out = max_pool2d(x + bias[c], 3, stride 2, pad 1) ; out_relu = relu(out)
 * Channels-last tensors: call the first two with (B*H*W, C, 1), the pool with channels_last = 1. */
/* Fused residual block of the 16-channel stage on the FP32 matrix cores, channels-last [B][H][W][16]:
 *   out = x + conv1(relu(conv0(relu(x)) + b0)) + b1 ; out_relu = relu(out)   (BinpackingNNet.py:21-27)
 * rp_nn_pack_conv16 reorders a contiguous [16][16][3][3] weight into the kernels' fragment order, [9 taps][64 lanes][4]:
 * frag[tap][lane][j] = W[co = lane & 15][ci = 4 * (lane >> 4) + j][tap] (a lane's four k-steps of a tap are four consecutive input
 * channels: one 16-byte load). */
int rp_nn_pack_conv16(rp_ctx *ctx, const float *w_dev, float *frag_dev);
/* Value head in one pass: out[b] = tanh(dot(z[b, :K], w) + bias[0])  (value_fc + tanh, BinpackingNNet.py:70,81); K a multiple of 4. */
int rp_nn_value_head(rp_ctx *ctx, const float *z_dev, const float *w_dev, const float *bias_dev, float *out_dev, int64_t B, int32_t K);
int rp_nn_resblock16(rp_ctx *ctx, const float *x_dev, const float *frag0_dev, const float *bias0_dev, const float *frag1_dev, const float *bias1_dev,
                     float *out_dev, float *out_relu_dev /* may be NULL */, int64_t B, int32_t H, int32_t W);
/* Both residual blocks of a 16-channel stage (ConvSequence.res_block0 then res_block1, BinpackingNNet.py:41-46) in one launch for
 * images of at most 128 pixels: frag4 = four rp_nn_pack_conv16 fragments (16-byte aligned) and bias4 = [4][16] in execution order
 * (block 0 conv0, conv1, block 1 conv0, conv1).  out_relu_dev may be NULL.  The product is taken transposed (weights x pixels), so
 * x, the skip operands and the result move as 16-byte pieces of the channels-last tensors; persistent waves. */
int rp_nn_resstage16(rp_ctx *ctx, const float *x_dev, const float *frag4_dev, const float *bias4_dev, float *out_dev, float *out_relu_dev, int64_t B,
                     int32_t H, int32_t W);
/* The same for a 32-channel stage on images of at most 80 pixels (5x5 at the 20x20 board).  rp_nn_pack_conv32 reorders a
 * contiguous [32][Cin][3][3] weight (Cin 16 or 32) into [9 taps][Cin / 16 halves][2 M tiles][64 lanes][4]:
 * frag[tap][h][mt][lane][j] = W[co = 16 mt + (lane & 15)][ci = Cin / 4 * (lane >> 4) + 4 h + j][tap];
 * frag4 = four of those (Cin 32, 16-byte aligned), bias4 = [4][32], in execution order. */
int rp_nn_pack_conv32(rp_ctx *ctx, const float *w_dev, float *frag_dev, int32_t Cin);
int rp_nn_resstage32(rp_ctx *ctx, const float *x_dev, const float *frag4_dev, const float *bias4_dev, float *out_dev, float *out_relu_dev, int64_t B,
                     int32_t H, int32_t W);
/* First convolution of a 32-channel stage + bias + max_pool2d(3, stride 2, pad 1) (ConvSequence.conv, BinpackingNNet.py:34,39-40)
 * on channels-last x [B][H][W][Cin] -> out [B][(H+1)/2][(W+1)/2][32]; Cin 16 (<= 112 pixels) or 32 (<= 80 pixels). */
int rp_nn_convpool32(rp_ctx *ctx, const float *x_dev, const float *frag_dev, const float *bias_dev, float *out_dev, int64_t B, int32_t Cin, int32_t H,
                     int32_t W);
int rp_nn_bias_relu(rp_ctx *ctx, float *x_dev, const float *bias_dev, int64_t B, int32_t C, int32_t HW);
int rp_nn_bias_residual(rp_ctx *ctx, const float *x_dev, const float *bias_dev, const float *res_dev, float *out_dev, float *out_relu_dev,
                        int64_t B, int32_t C, int32_t HW);
int rp_nn_bias_pool(rp_ctx *ctx, const float *x_dev, const float *bias_dev, float *out_dev, float *out_relu_dev, int64_t B, int32_t C, int32_t H,
                    int32_t W, int32_t channels_last);
/* Host copy of the waiting leaves' packed states and slots (parity tests, host evaluators). */
int rp_leaf_states(rp_ctx *ctx, int32_t max_rows, uint64_t *rows_out /*[n][H]*/, uint8_t *remaining_out /*[n][N]*/,
                   int32_t *slot_out /*[n]*/, int32_t *n_out);
/* Expansion + backup: masks and renormalises pi with the leaf's valid moves (MCTS_bpp.py:88-100,
 * float64, NumPy summation order), stores Vs/Ns (:102-103) and backs v up the path (:130-139).
 * pi_dev [n][W*N] and v_dev [n] are DEVICE float32 (probabilities, i.e. exp(log_softmax), NNet.py:85),
 * row b belonging to the b-th waiting leaf.  pi must be what NNet.predict returns -- probabilities, pi >= 0: for a node with more
 * than 64 legal moves the search keeps "the unvisited move with the largest pi (lowest action among equals)" as the one PUCT
 * candidate of all unvisited moves, which is the reference's argmax over them exactly when cpuct > 0 and pi >= 0. */
int rp_commit_eval(rp_ctx *ctx, const float *pi_dev, const float *v_dev);
/* The same from the policy head's raw outputs (logits_fc, BinpackingNNet.py:69,79): the softmax of NNet.predict (NNet.py:81-85:
 * exp(log_softmax(x))) is taken inside the kernel, float32, exp(x - max) / sum -- no separate softmax pass over [n][W*N].
 * W * N <= 1536 (a lane keeps its 24 elements of the row in registers); larger action spaces are refused with RP_ERR_ARG and go
 * through rp_commit_eval_logits_wide, or take the softmax first and call rp_commit_eval. */
int rp_commit_eval_logits(rp_ctx *ctx, const float *logits_dev, const float *v_dev);
/* The same contract for every geometry the engine accepts (W * N <= 8192): the wave stages the row in LDS and makes its passes there,
 * one wave per workgroup (rp_debug_commit_plan).  The arithmetic, float32, in this order: m = max of the row; e[a] = expf(x[a] - m);
 * lane l adds the e of a = l, l + 64, l + 128, ... in ascending order, the 64 lane sums are combined by the xor butterfly with
 * offsets 32, 16, ... 1; p[a] = e[a] / sum, one division per element.  rp_commit_eval_logits computes exactly that, so where both
 * apply (W * N <= 1536) the two calls leave bit-identical trees. */
int rp_commit_eval_logits_wide(rp_ctx *ctx, const float *logits_dev, const float *v_dev);
/* Same with HOST float32 buffers (tests, CPU evaluators). */
int rp_commit_eval_host(rp_ctx *ctx, const float *pi_host, const float *v_host, int32_t n_rows);

/* ---- network-free evaluator: uniform random playouts in place of nnet.predict (MCTS_bpp.py:87) ---- */
/* Playout j from state S = (rows, remaining) of the episode with id e draws from h0 = mix64(key_hash(S, seed) ^ e): key_hash is the
 * sequential splitmix64 over the salt (here rp_config.seed), the H row masks, then the remaining-item words -- the hash of the tie
 * rule.  At step s = 0, 1, ... it counts the legal moves nv (getValidMoves, BinPackingGame.py:78-92); nv == 0 ends the playout,
 * otherwise it plays legal move number umulhi(sample(h0, j, s), nv) in ascending action order (a = item * W + column) through
 * execute_move (BinPackingLogic.py:95-109), sample(seed, episode, move) being the RP_MOVE_SAMPLE stream
 * mix64(mix64(mix64(seed) ^ episode) ^ move).  Every move places one item, so a playout has at most N steps.  Its outcome is
 * getRankedReward (BinPackingGame.py:188-212) of the final bin against the episode's R2 threshold, total area and max_h, the r == bl
 * tie resolved from the final state and rp_config.tie_salt exactly as the search resolves Es; its score is r.  A function of (state,
 * episode items, episode id, threshold, seed, tie salt) only: not of the slot, the evaluator row, the group or the launch. */
/* MCTS_bpp.py:87 for the leaves waiting for evaluation: v_dev[b] = float32(sum of the `playouts` outcomes) / float32(playouts), row b as
 * in rp_leaf_planes, and -- when pi_dev != NULL -- pi_dev row b = float32(1) / float32(W * N) in every entry (the uniform prior;
 * rp_commit_eval masks and renormalises it).  DEVICE float32 buffers of capacity_rows rows.  Enqueues one kernel only: capturable.
 * 1 <= playouts <= 256, else RP_ERR_ARG.  Under a rollout prior other than (0, 0, 0) the rows of pi_dev are the prior's and one more
 * kernel is enqueued (rp_set_rollout_prior below). */
int rp_rollout_eval(rp_ctx *ctx, int32_t playouts, float *pi_dev /* may be NULL */, float *v_dev, int64_t capacity_rows);
/* The same playouts (MCTS_bpp.py:87) over a batch of B host states, `playouts` each, with everything they produce: the resolved outcome
 * (+-1), the score r, the moves played (0 for a state without a legal move) and the final bin's row masks (board_out may be NULL).
 * episode_id NULL: every state plays as episode 0; rewards / alpha: the R2 buffer shared by the batch, as rp_game_ended takes it. */
int rp_rollout_states(rp_ctx *ctx, int64_t B, const uint64_t *rows, const uint8_t *remaining, const uint8_t *item_wh,
                      const int32_t *total_area, const int32_t *max_h, const uint64_t *episode_id /* NULL: 0 */,
                      const double *rewards, int32_t n_rewards, double alpha, int32_t playouts,
                      int32_t *outcome_out /*[B][playouts]*/, double *score_out, int32_t *moves_out, uint64_t *board_out /*[B][playouts][H]*/);
/* The action lists of the playouts rp_rollout_states plays (MCTS_bpp.py:87) for the same states, episode ids and seed, through the
 * recording path of the playout incumbents (rp_set_incumbent_playouts): action_out[b][j][s] = item * W + column of step s of playout j as
 * getNextState takes it (BinPackingGame.py:58-76), zero for s >= moves_out[b][j].  Replayed from the state they end on the board
 * rp_rollout_states returns, whose score is BinPackingGame.py:188-212. */
int rp_rollout_paths(rp_ctx *ctx, int64_t B, const uint64_t *rows, const uint8_t *remaining, const uint8_t *item_wh,
                     const uint64_t *episode_id /* NULL: 0 */, int32_t playouts, uint16_t *action_out /*[B][playouts][N]*/,
                     int32_t *moves_out /*[B][playouts]*/);
/* The playout policy of the context: how a playout (MCTS_bpp.py:87) chooses among the legal moves (getValidMoves,
 * BinPackingGame.py:78-92).  Two small integer powers (w_pow, h_pow); a legal move of item i with size (w_i, h_i) gets the integer
 * weight wt_i = w_i^w_pow * h_i^h_pow.  The default (0, 0) is the uniform rule above.  The sampling rule:
 *   - At step s of playout j, m_i is the legal-column mask of item i and c_i = popcount(m_i).
 *   - nv = sum c_i == 0 ends the playout.
 *   - Otherwise T = sum c_i * wt_i.
 *   - pick = umulhi(sample(h0, j, s), T), the same stream: h0 = mix64(key_hash(S, seed) ^ e).
 *   - The legal moves lie in ascending action order (a = item * W + column).  Each move occupies wt_i consecutive units of [0, T).
 *     The move that owns unit `pick` is played:
 *       item   = the first i whose inclusive sum sum_{k<=i} c_k wt_k exceeds pick;
 *       column = set bit number floor((pick - sum_{k<i} c_k wt_k) / wt_i) of m_i, counted from 0.
 *   - Limits: w_pow >= 0, h_pow >= 0, w_pow + h_pow <= 2.  Then 1 <= wt_i <= 4096 and T <= 64 * 128 * 4096 = 2^25, so the sums stay
 *     in 32 bits.
 *   - With (0, 0) the rule is the uniform one, bit for bit.
 * Everything else about a playout is unchanged: its outcome, its score, the tie rule, the independence from slot, row and launch, and the
 * bound of N steps.  The weights look at the item alone -- not at the column or the height the move would reach -- so they are a
 * function of the episode's items and cost no state per slot.
 * RP_ERR_ARG outside the limits; RP_ERR_STATE while any slot is in the middle of an episode (an incumbent's record would stop being a
 * function of the search alone: a playout offer is replayed under the policy that scored it).  Applies to rp_rollout_eval,
 * rp_rollout_states, rp_rollout_paths and the playout offers from then on.  Kernel arguments are baked into captured graphs:
 * re-capture after switching. */
int rp_set_playout_policy(rp_ctx *ctx, int32_t w_pow, int32_t h_pow);
/* The powers in force (either pointer may be NULL). */
int rp_playout_policy(const rp_ctx *ctx, int32_t *w_pow_out, int32_t *h_pow_out);
/* The landing power of the playouts: a setting of its own beside the playout policy, land_pow in {0, 1, 2}, default 0.  It lets a
 * playout (MCTS_bpp.py:87) weigh a legal move by the row it lands on as well as by its item.  At step s of playout j, on the
 * playout's current board:
 *   - m_i is the legal-column mask of item i (getValidMoves, BinPackingGame.py:78-92).  No legal move ends the playout.
 *   - wt_i = w_i^w_pow * h_i^h_pow comes from the playout policy in force, unchanged.
 *   - L(i, c) = (H - t(w_i, c))^land_pow, t(w, c) the first row whose window [c, c + w) is empty, H - 1 if none is: the t of the
 *     rollout prior below (BinPackingLogic.py:66-68).  1 <= L <= 4096.
 *   - R_i = sum of L(i, c) over c in m_i <= 64 * 4096 = 2^18.  S_i = wt_i * R_i <= 2^30.
 *   - T = sum S_i <= 128 * 2^30 = 2^37: a 64-bit integer sum.
 *   - pick = umulhi(sample(h0, j, s), T), the same stream: h0 = mix64(key_hash(S, seed) ^ e).
 *   - item   = the first i whose inclusive sum sum_{k<=i} S_k exceeds pick;
 *     q      = floor((pick - sum_{k<i} S_k) / wt_i), so q < R_i;
 *     column = the first legal column c of the item, ascending, whose inclusive sum of L(i, .) over the item's legal columns up to c
 *              exceeds q.
 *     Equivalently, each move owns wt_i * L(i, c) consecutive units of [0, T) in ascending action order.
 *   - With land_pow == 0, L = 1: the rule of the playout policy above, bit for bit.
 * Everything else about a playout is unchanged: h0, its outcome and score, the tie rule, the bound of N steps, the independence from
 * slot, row and launch, and the replay of a winning playout in the playout offers under the setting that scored it.
 * RP_ERR_ARG outside 0..2; RP_ERR_STATE while any slot is in the middle of an episode, as rp_set_playout_policy; a refused call changes
 * nothing.  Applies to rp_rollout_eval, rp_rollout_states, rp_rollout_paths and the playout offers from then on.  Kernel arguments are
 * baked into captured graphs: re-capture after switching. */
int rp_set_playout_landing(rp_ctx *ctx, int32_t land_pow);
/* The power in force (the pointer may be NULL). */
int rp_playout_landing(const rp_ctx *ctx, int32_t *land_pow_out);
/* The rollout prior of the context: the pi that rp_rollout_eval returns in place of nnet.predict's (MCTS_bpp.py:87).  Three small
 * integer powers (w_pow, h_pow, land_pow).  The default (0, 0, 0) is the uniform prior above.  The rule:
 *   - For a leaf state, m_i is the legal-column mask of item i (getValidMoves, BinPackingGame.py:78-92).
 *   - A legal move (i, c) gets the integer weight u(i, c) = w_i^w_pow * h_i^h_pow * (H - t(i, c))^land_pow.
 *   - t(i, c) is the first row r, counted from 0, whose window [c, c + w_i) is empty: the t of get_adjacency
 *     (BinPackingLogic.py:66-68), and, where an empty row exists, the row execute_move fills first (BinPackingLogic.py:103-105).
 *     If no row of the window is empty, t = H - 1: the reference's `for` falls through.  Such moves exist, legality only counts cells
 *     (BinPackingLogic.py:89).  So 1 <= H - t <= H: a move that lands low weighs more.
 *   - Limits: w_pow, h_pow, land_pow >= 0, w_pow + h_pow <= 2, land_pow <= 2.  Then 1 <= u <= 4096 * 4096 = 2^24, which float32
 *     holds exactly, and T = sum of u over all legal moves <= 8192 * 2^24 = 2^37: a 64-bit integer sum, whose value does not depend
 *     on the summation order.
 *   - pi[a] = float32(float64(u) / float64(T)) at the legal actions a = i * W + c -- one IEEE double division, rounded once to
 *     float32 -- and 0.0f everywhere else.  A state without a legal move gives an all-zero row.
 *   - With (0, 0, 0) the row is float32(1) / float32(W * N) in every entry, bit for bit what it was before the prior existed.
 * rp_commit_eval masks and renormalises the row as it does any pi (MCTS_bpp.py:88-100); the row is non-negative, so the candidate
 * rule for more than 64 legal moves (rp_commit_eval above) keeps holding.
 * RP_ERR_ARG outside the limits; RP_ERR_STATE while any slot is in the middle of an episode (a search stays a function of one setting).
 * From then on, while the prior is not (0, 0, 0): rp_rollout_eval writes pi_dev row b = the row above of the b-th waiting leaf, the row
 * mapping of v_dev (compact rows included); pi_dev == NULL is RP_ERR_ARG, the prior has no other way out; the call enqueues two
 * kernels and stays capturable.  Under (0, 0, 0) nothing about rp_rollout_eval changes.  Kernel arguments are baked into captured
 * graphs: re-capture after switching. */
int rp_set_rollout_prior(rp_ctx *ctx, int32_t w_pow, int32_t h_pow, int32_t land_pow);
/* The powers in force (any pointer may be NULL). */
int rp_rollout_prior(const rp_ctx *ctx, int32_t *w_pow_out, int32_t *h_pow_out, int32_t *land_pow_out);
/* The prior rows of a batch of B host states under the prior in force, stateless like rp_rollout_states: pi_out row b is the row
 * above for state b (float32(1) / float32(W * N) in every entry under (0, 0, 0)). */
int rp_rollout_prior_states(rp_ctx *ctx, int64_t B, const uint64_t *rows, const uint8_t *remaining, const uint8_t *item_wh,
                            float *pi_out /* HOST [B][W*N] */);

/* ---- results ------------------------------------------------------------------------- */
/* counts[a] = Nsa[(root, a)] (MCTS_bpp.py:40-41), host buffer [count][W*N] */
int rp_root_counts(rp_ctx *ctx, int32_t first, int32_t count, uint32_t *counts_out);
/* phase_out / sims_done_out / moves_out / episode_out: host buffers [count] (any may be NULL) */
int rp_game_status(rp_ctx *ctx, int32_t first, int32_t count, int32_t *phase_out, int32_t *sims_done_out,
                   int32_t *moves_out, uint64_t *episode_out);
/* Return value of each slot's latest simulation (MCTS.search returns v, MCTS_bpp.py:83,104,139) and its kind. */
int rp_last_values(rp_ctx *ctx, int32_t first, int32_t count, double *v_out, int32_t *kind_out);
/* Plays `action[i]` in slot first+i (CoachBPP.py:88-91): the child becomes the root, the tree is
 * kept; ended_out[i] = 0 / +-1 as getGameEnded, score_out[i] = r.  Only with RP_MOVE_EXTERNAL; RP_ERR_STATE under RP_MOVE_INCUMBENT,
 * whose line an outside move would leave. */
int rp_advance_roots(rp_ctx *ctx, int32_t first, int32_t count, const int32_t *action, int32_t *ended_out,
                     double *score_out);
/* Finished episodes since the last call (auto move rules): up to max_n records, oldest first. */
int rp_pop_finished(rp_ctx *ctx, int64_t max_n, uint64_t *episode_id_out, int32_t *outcome_out, double *score_out,
                    int32_t *moves_out, int64_t *n_out);
/* rp_pop_finished plus each episode's packing (rp_set_trace): the moves CoachBPP.executeEpisode / arena_playing played through
 * getNextState (CoachBPP.py:88-91, 262) and the board it ended on.  action_out[k][m] / rows_out[k][m] describe move m of record k
 * (zero for m >= moves_out[k]), board_out[k][r] is row r of the final bin.  Same ring and cursor as rp_pop_finished; any output may be
 * NULL.  RP_ERR_ARG while the trace is off. */
int rp_pop_finished_packings(rp_ctx *ctx, int64_t max_n, uint64_t *episode_id_out, int32_t *outcome_out, double *score_out,
                             int32_t *moves_out, uint16_t *action_out /*[max_n][N]*/, uint64_t *rows_out /*[max_n][N]*/,
                             uint64_t *board_out /*[max_n][H]*/, int64_t *n_out);
/* rp_pop_finished_packings plus each episode's incumbent (rp_set_incumbent: the terminals of MCTS_bpp.py:78-83, scored by
 * BinPackingGame.py:188-212): best_action_out[k][m] is move m of record k's incumbent from the episode's initial state (zero for
 * m >= best_moves_out[k]), best_board_out[k][r] row r of its bin.  Same ring and cursor as rp_pop_finished; any output may be NULL.
 * RP_ERR_ARG while incumbents are off, and when action_out / rows_out / board_out is requested while the trace is off. */
int rp_pop_finished_best(rp_ctx *ctx, int64_t max_n, uint64_t *episode_id_out, int32_t *outcome_out, double *score_out, int32_t *moves_out,
                         uint16_t *action_out /*[max_n][N]*/, uint64_t *rows_out /*[max_n][N]*/, uint64_t *board_out /*[max_n][H]*/,
                         double *best_score_out, int32_t *best_outcome_out, int32_t *best_moves_out, int32_t *best_prefix_out,
                         int32_t *best_updates_out, uint16_t *best_action_out /*[max_n][N]*/, uint64_t *best_board_out /*[max_n][H]*/,
                         int64_t *n_out);
/* Running incumbents of slots first .. first + count - 1 as host copies (the Es terminals of MCTS_bpp.py:78-83 seen so far in each
 * slot's episode, scored by BinPackingGame.py:188-212): moves_out = -1, and zeros elsewhere, where the episode has none yet.  Any output
 * may be NULL.  RP_ERR_ARG while incumbents are off. */
int rp_incumbents(rp_ctx *ctx, int32_t first, int32_t count, double *score_out, int32_t *outcome_out, int32_t *moves_out,
                  int32_t *prefix_out, int32_t *updates_out, uint16_t *action_out /*[count][N]*/, uint64_t *board_out /*[count][H]*/);
/* rp_pop_finished_best plus where each incumbent came from (rp_set_incumbent_playouts): best_tree_moves_out[k] = the number of actions
 * after which the search tree was left -- for a playout of MCTS_bpp.py:87 the played moves plus the leaf's path, its own moves
 * (BinPackingGame.py:58-76) follow in best_action_out[k]; for a tree terminal all of best_moves_out[k] -- and best_playout_out[k] = the
 * playout's index, -1 for a tree terminal (scores: BinPackingGame.py:188-212).  Same ring and cursor as rp_pop_finished; any output may
 * be NULL.  RP_ERR_ARG while playout incumbents are off, and for a trace output while the trace is off. */
int rp_pop_finished_best_playouts(rp_ctx *ctx, int64_t max_n, uint64_t *episode_id_out, int32_t *outcome_out, double *score_out,
                                  int32_t *moves_out, uint16_t *action_out /*[max_n][N]*/, uint64_t *rows_out /*[max_n][N]*/,
                                  uint64_t *board_out /*[max_n][H]*/, double *best_score_out, int32_t *best_outcome_out,
                                  int32_t *best_moves_out, int32_t *best_prefix_out, int32_t *best_updates_out,
                                  uint16_t *best_action_out /*[max_n][N]*/, uint64_t *best_board_out /*[max_n][H]*/,
                                  int32_t *best_tree_moves_out, int32_t *best_playout_out, int64_t *n_out);
/* The companion of rp_incumbents: (tree_moves, playout) of the running incumbents of slots first .. first + count - 1 -- a playout of
 * MCTS_bpp.py:87 (its moves: BinPackingGame.py:58-76, its score: BinPackingGame.py:188-212) or, with playout = -1, a tree terminal;
 * (0, -1) where the episode has none yet.  Either output may be NULL.  RP_ERR_ARG while playout incumbents are off. */
int rp_incumbent_sources(rp_ctx *ctx, int32_t first, int32_t count, int32_t *tree_moves_out, int32_t *playout_out);
/* Engine counters summed over slots since create/reset: [0] simulations, [1] expansions (leaf evaluations),
 * [2] terminal returns, [3] path edges walked, [4] sum of n_valid at selected nodes, [5] sum of n_valid at
 * expanded leaves, [6] transposition links, [7] nodes created, [8] moves played, [9] episodes finished,
 * [10] hash probes (64-slot windows), [11] key bytes compared, [12] sum of visited edges at selected nodes,
 * [13] visited-edge entries created, [14] moves that followed the incumbent (RP_MOVE_INCUMBENT; 0 under every other rule),
 * [15] reserved. */
int rp_counters(rp_ctx *ctx, int64_t *out16, int32_t reset);

/* ---- replay buffer (CoachBPP.executeEpisode's trainExamples, CoachBPP.py:80,99) -------- */
/* Number of examples recorded so far. */
int rp_examples_count(rp_ctx *ctx, int64_t *n_out);
/* Dense training tensors for examples [first, first+count): planes FP32 [count][N+1][H][W],
 * pi FP32 [count][W*N] (= counts / sum, MCTS_bpp.py:51-54), value FP32 [count] (the episode's ranked
 * outcome, 0 while the episode is unfinished) -- DEVICE buffers. */
int rp_examples_tensors(rp_ctx *ctx, int64_t first, int64_t count, float *planes_dev, float *pi_dev, float *value_dev);
/* Episode id and move number (0-based) of examples [first, first+count) -- HOST buffers.  The buffer fills in completion
 * order across slots; the reference appends episode by episode, move by move (CoachBPP.py:80,133), so callers sort by
 * (episode, move) before they trim to maxlenOfQueue (CoachBPP.py:122). */
int rp_examples_meta(rp_ctx *ctx, int64_t first, int64_t count, uint64_t *episode_id_out, int32_t *move_out);
int rp_examples_clear(rp_ctx *ctx);
/* The replay buffer in its PACKED form -- what ranks exchange and what the history of CoachBPP.learn keeps (CoachBPP.py:152-157), ~0.4 KB
 * per example at 20x20 / 32 items where the dense training tensors of rp_examples_tensors take 55 KB:
 *   key      u32 [E][KW]    the recorded state as the engine keys it: H row masks (u32 for W <= 32, else u64) then ceil(N / 32) words of
 *                           remaining-item bits (KW = H * (W > 32 ? 2 : 1) + ceil(N / 32), rounded up to even when W > 32)
 *   item_wh  u8  [E][N][2]  the episode's item sizes (getInitItems, BinPackingGame.py:37-51)
 *   value    i32 [E]        the episode's ranked outcome (CoachBPP.py:99)
 *   sp_off / sp_n i32 [E]   first entry and number of entries of the example's visit counts in the pool
 *   sp_act u16 / sp_cnt u32 [S]   pool of (action, Nsa) pairs, one per visited root edge (counts of MCTS_bpp.py:40-41; a one-hot (a, 1) for
 *                           greedy examples, :43-49)
 *   episode i64 / move i32 [E]    may be NULL
 * rp_examples_packed_count returns E and S; rp_examples_packed copies everything recorded so far into caller-owned DEVICE buffers of
 * those sizes (device-to-device, on the context's stream). */
int rp_examples_packed_count(rp_ctx *ctx, int64_t *n_examples_out, int64_t *n_sparse_out);
int rp_examples_packed(rp_ctx *ctx, int64_t n_examples, int64_t n_sparse, uint32_t *key_dev, uint8_t *item_wh_dev, int32_t *value_dev,
                       int32_t *sp_off_dev, int32_t *sp_n_dev, uint16_t *sp_act_dev, uint32_t *sp_cnt_dev, int64_t *episode_dev, int32_t *move_dev);
/* Training minibatch out of a packed replay set (the examples argument of NNetWrapper.train, NNet.py:27-67, picked by the index draw of
 * :43): row k of the outputs = example index_dev[k] (NULL: example k) of the caller-owned packed arrays above (sp_off 64-bit here: sets
 * gathered from several ranks and iterations outgrow 32 bits), expanded exactly like rp_examples_tensors.  Stateless: uses only the
 * context's geometry and stream. */
int rp_expand_examples(rp_ctx *ctx, int64_t n, const int64_t *index_dev, int64_t n_examples /* E */, int64_t n_sparse /* S */, const uint32_t *key_dev,
                       const uint8_t *item_wh_dev, const int32_t *value_dev, const int64_t *sp_off_dev, const int32_t *sp_n_dev,
                       const uint16_t *sp_act_dev, const uint32_t *sp_cnt_dev, float *planes_dev, float *pi_dev, float *value_out_dev);
/* Every index is checked on the device against E and S (an index list or a pool entry outside the arrays yields a zero row, never a
 * stray access); rp_check synchronises the context's stream and returns the first error device code recorded since the last check
 * (RP_ERR_ARG for such an index, RP_ERR_CAPACITY for an arena overflow), like every synchronising call does.
 *
 * Device errors (tests/test_gpu_capacity.py holds the engine to every clause):
 *  - A kernel that cannot go on records a code; the FIRST code recorded since the last report is kept.  It is returned -- with
 *    rp_last_error naming the cause -- by the next call that looks for it (rp_check, rp_game_status, rp_search_step with
 *    n_leaves_out, rp_advance_roots, rp_begin_episodes, rp_begin_pool among them), and by that call only: reporting clears it, the
 *    call after it returns RP_OK again unless another error has been recorded since.
 *  - RP_ERR_CAPACITY "node arena" / "legal-move arena" / "visited-edge arena": a slot needed a node beyond node_cap, a run of legal
 *    moves or a block of visited edges for which its arena had no chunk left.  The caps are exact: an episode whose tree has n nodes
 *    runs in node_cap = n and fails in n - 1; one whose arenas peak at (P, V) chunks (rp_arena_peak) runs in edge_cap = P chunks and
 *    vis_cap = V chunks and fails with one chunk fewer in either.  RP_ERR_ASSERT: rp_advance_roots got an action that is no legal move
 *    of its slot's root.  In both cases the slot is left RP_PHASE_FAILED and takes no further part in rp_search_step; nothing is
 *    written outside the slot's own arenas, every other slot goes on and computes exactly what it computes without the failure.
 *    rp_begin_episodes on the slot (or rp_begin_pool) starts it afresh, with a tree like any other's.
 *  - RP_ERR_CAPACITY "finished-episode ring": episodes ended while the ring already held its max(4 * games, 1024) records.  Their
 *    records are lost (each reports), the records in the ring stay valid and are popped as usual; the slots go on, and once the ring
 *    has been popped empty it records again.
 *  - RP_ERR_CAPACITY "replay buffer": an example found no room.  Past max_examples it is lost: rp_examples_count stays at
 *    max_examples, the examples recorded before it are intact, and each of them receives the outcome of its own episode and of no
 *    other.  When only the pool of (action, count) pairs (max_sparse) is full the example is kept without pairs (sp_n = 0, an all-zero
 *    pi).  The episodes go on.  After rp_examples_clear the buffer records again like one that never overflowed. */
int rp_check(rp_ctx *ctx);

/* ---- inspection (parity tests) --------------------------------------------------------- */
/* Sizes of slot g's tree: nodes in use and the span of its legal-move arena (the index range of rp_dump_tree's edge arrays). */
int rp_tree_size(rp_ctx *ctx, int32_t slot, int32_t *n_nodes_out, int32_t *n_edges_out);
/* High-water marks of the level arenas over all slots since create: chunks in use (legal-move runs, visited blocks) and
 * the chunk sizes in entries (6 and 32 bytes per entry).  Sizing aid for edge_cap / vis_cap: the same episodes run in exactly that
 * many chunks of each kind and in no fewer (see "device errors" at rp_check). */
int rp_arena_peak(rp_ctx *ctx, int32_t *prior_chunks_out, int32_t *visited_chunks_out, int32_t *chunk_entries_out2);
/* Host copy of slot g's tree.  Node i: rows u64[H], remaining u8[N], term i8 (0 / +-1 = Es),
 * term_kind u8, expanded u8, ns u32, edge_off u32, n_valid u32.  Edge e (one per legal move, dense view of the sparse
 * device layout): action u16, P f64, Q f64, nsa u32, q_kind u8, child u32 (0xFFFFFFFF = not linked yet). */
int rp_dump_tree(rp_ctx *ctx, int32_t slot, uint64_t *node_rows, uint8_t *node_remaining, int8_t *node_term,
                 uint8_t *node_term_kind, uint8_t *node_expanded, uint32_t *node_ns, uint32_t *node_edge_off,
                 uint32_t *node_n_valid, uint16_t *edge_action, double *edge_p, double *edge_q, uint32_t *edge_nsa,
                 uint8_t *edge_q_kind, uint32_t *edge_child);
/* Launch plan of rp_commit_eval_logits_wide for A actions, n_leaves blocks of the pairwise sum over A and G slots on a device with
 * lds_per_cu bytes of LDS per CU -- host arithmetic only, no context and no device.  out[8]: waves per workgroup, LDS bytes per
 * workgroup, grid, block, then one wave's parts in bytes: row, block sums, terms, mask.  0: fits; 1: bad argument; 2: the
 * workgroup's LDS exceeds lds_per_cu (out is filled in). */
int rp_debug_commit_plan(int32_t A, int32_t n_leaves, int64_t G, int64_t lds_per_cu, int64_t *out);
/* Device self-tests used by the GPU parity suite: sqrt / Q-update / NumPy-order sum on device,
 * host buffers in and out. */
int rp_selftest_sqrt(rp_ctx *ctx, int64_t n, double *sqrt_n_out, double *sqrt_n_eps_out);
int rp_selftest_q_update(rp_ctx *ctx, int64_t n, const double *q, const uint8_t *q_kind, const uint32_t *nsa,
                         const double *v, const uint8_t *v_kind, double *q_out, uint8_t *q_kind_out);
int rp_selftest_masked_prior(rp_ctx *ctx, int64_t B, const float *pi /*[B][A]*/, const uint8_t *valid /*[B][A]*/,
                             double *p_out /*[B][A]*/);
/* The softmax that rp_commit_eval_logits (wide == 0: the row in registers, RP_ERR_ARG beyond 1536 actions) and rp_commit_eval_logits_wide
 * (wide != 0: the row in LDS, every action space) take inside the commit kernel, from the same device helpers in the same order, one wave
 * per row; tests/test_gpu_commit_wide.py holds the commit kernel's priors to it bit for bit. */
int rp_selftest_softmax(rp_ctx *ctx, int64_t B, const float *logits /*[B][A]*/, int32_t wide, float *pi_out /*[B][A]*/);

#ifdef __cplusplus
}
#endif
#endif
