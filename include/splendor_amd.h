/*
 * splendor_amd.h — C ABI of the MI355X-native Splendor engine (libsplendor_amd.so).
 *
 * Drop-in boundary for the reference's Game plug-in surface as it is used on the
 * self-play hot path (kuboyoo/alphazero-general-ori):
 *   Game API          Game.py:14-162, implemented by SplendorGame.py:11-86
 *   rules engine      SplendorLogicNumba.Board (@jitclass), SplendorLogicNumba.py:84-774
 * The reference binds these from Python one board at a time through Numba's jitclass
 * boxing; this library exposes the same operations BATCHED over B boards held in device
 * memory (HBM), stream-ordered, with no allocation in any hot call. The Python host
 * mirror (alphazero-general-ori_amd/splendor/SplendorGame.py) binds it with ctypes.
 *
 * Conventions
 *   - All array arguments are DEVICE pointers owned by the caller unless noted.
 *   - state: B boards x S bytes, S = 7*R, R = 32 + 10n + n^2 (the reference's int8 (R,7)
 *     observation, row-major, identical bytes to board.tobytes(), SplendorGame.py:63-64).
 *   - mask: B x 7 uint64; bit (a % 64) of word (a / 64) is action a (0..408).
 *   - player arrays are int8 (0..n-1); a NULL player pointer means "player 0 everywhere".
 *   - chance: either explicit uniforms (u != NULL: board b consumes u[b*u_stride + k],
 *     k = 0,1,.. in the reference's draw order) or counter-based Philox4x32-10 with
 *     key = seed: uniform k is half (k & 1) of the block at counter
 *     (k >> 1, board_base + b, stream, 'SPLD'), 53 bits from words (0,1) or (2,3).
 *   - hip_stream: a hipStream_t (NULL = default stream).
 *   - Return value: 0 ok; SPL_EINVAL bad argument; SPL_EDEVICE HIP launch/runtime error.
 *     Per-board errors found on device (action out of range) are OR-ed into *err when
 *     err != NULL (device int32), so hot calls never synchronise.
 */
#ifndef SPLENDOR_AMD_H
#define SPLENDOR_AMD_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SPL_ABI_VERSION 11
#define SPL_ACTIONS 409
#define SPL_MASK_WORDS 7
#define SPL_EINVAL (-1)
#define SPL_EDEVICE (-2)
#define SPL_ERR_BAD_ACTION 1
#define SPL_ERR_BAD_INDEX 2

typedef struct spl_ctx spl_ctx;

int spl_abi_version(void);

/* Board(num_players) rule constants (SplendorLogicNumba.py:86-98): n in {2,3,4};
 * token_limit = NUM_TOKEN_LIMIT (default 10; Board.setNumTokenLim, :214-215). */
int spl_ctx_create(int n_players, int token_limit, spl_ctx **out);
int spl_ctx_destroy(spl_ctx *ctx);
/* Board.setNumTokenLim (SplendorLogicNumba.py:214-215; Arena.py:116 handicap games) */
int spl_ctx_set_token_limit(spl_ctx *ctx, int token_limit);
/* Rule switches of the context: a bit set of SPL_RULE_* flags, 0 (the full game) after create.
 * SPL_RULE_NO_RESERVE is the reference's ENABLE_ACTION_RESERVE = False (SplendorGame.
 * disableReserve, SplendorGame.py:82-83; SplendorLogicNumba.py:96,508-510): _valid_reserve(
 * is_limit=True) is empty, so actions 12..26 (reserve a visible card / from a deck) are never
 * legal. Nothing else reads the switch: reserve + give one (290..364, _valid_exchange's
 * is_limit=False call, :260) stays legal, pass (408) is still legal iff nothing else is (:263),
 * and make_move, scores, end checks, chance and symmetries are unchanged. The mask under the
 * rule is therefore the full mask with bits 12..26 cleared, then bit 408 set iff bits 0..407
 * are empty. Every call that builds a legality mask from the context honours the flags at
 * launch time: spl_valid_moves, spl_player_move, spl_rollout_step / _run, spl_playout / _seq.
 * A search handle copies the context's rules (as its token limit) in spl_mcts_create and keeps
 * them for its lifetime: trees store masks, so later changes of the context do not reach it.
 * set_rules: SPL_EINVAL on a NULL context or unknown bits (nothing is changed); the token limit
 * is untouched, and spl_ctx_set_token_limit leaves the flags alone. spl_ctx_rules /
 * spl_mcts_rules return the flags (SPL_EINVAL on NULL). */
#define SPL_RULE_NO_RESERVE 1
int spl_ctx_set_rules(spl_ctx *ctx, int flags);
int spl_ctx_rules(const spl_ctx *ctx);
/* observation_size (SplendorLogicNumba.py:26-27): rows R; bytes per board 7*R */
int spl_state_rows(const spl_ctx *ctx);
int spl_state_bytes(const spl_ctx *ctx);

/* Board.init_game (SplendorLogicNumba.py:222-246) / SplendorGame.getInitBoard
 * (SplendorGame.py:17-19). Writes B fresh boards; player_out (nullable) set to 0.
 * Draws: 12 cards x 2 uniforms, then n+1 noble draws (partial Fisher-Yates). */
int spl_init(const spl_ctx *ctx, int B, int8_t *state, int8_t *player_out,
             const double *u, int u_stride, uint64_t seed, uint32_t stream,
             uint32_t board_base, void *hip_stream);

/* SplendorGame.getValidMoves (SplendorGame.py:35-37) -> Board.valid_moves
 * (SplendorLogicNumba.py:251-265). */
int spl_valid_moves(const spl_ctx *ctx, int B, const int8_t *state, const int8_t *player,
                    uint64_t *mask_out, void *hip_stream);

/* SplendorGame.getNextState (SplendorGame.py:30-33) -> Board.make_move
 * (SplendorLogicNumba.py:267-289), in place on `state`. deterministic=1 is the in-tree
 * transition (no deck draws, MCTS.py:228). next_player_out nullable. */
int spl_step(const spl_ctx *ctx, int B, int8_t *state, const int8_t *player,
             const int16_t *action, int8_t *next_player_out, int deterministic,
             const double *u, int u_stride, uint64_t seed, uint32_t stream,
             uint32_t board_base, int32_t *err, void *hip_stream);

/* SplendorGame.getGameEnded (SplendorGame.py:39-41) -> Board.check_end_game
 * (SplendorLogicNumba.py:320-334). out: B x n float32. */
int spl_game_ended(const spl_ctx *ctx, int B, const int8_t *state, float *out,
                   void *hip_stream);

/* SplendorGame.getCanonicalForm (SplendorGame.py:51-57) -> Board.swap_players
 * (SplendorLogicNumba.py:338-347). out may equal state. */
int spl_canonical(const spl_ctx *ctx, int B, const int8_t *state, const int8_t *player,
                  int8_t *out, void *hip_stream);

/* SplendorGame.getScore / getRound (SplendorGame.py:43-49): out B x n int32 / B int32 */
int spl_score(const spl_ctx *ctx, int B, const int8_t *state, int32_t *out, void *hip_stream);
int spl_round(const spl_ctx *ctx, int B, const int8_t *state, int32_t *out, void *hip_stream);

/* In-tree transition of MCTS.get_next_best_action_and_canonical_state (MCTS.py:222-237):
 * child = swap_players(make_move(copy(parent), a, 0, deterministic=True)). */
int spl_tree_step(const spl_ctx *ctx, int B, const int8_t *parent, const int16_t *action,
                  int8_t *child, int32_t *err, void *hip_stream);

/* The rule-based players of SplendorPlayers.py (RandomPlayer :13-21, GreedyPlayer :92-112)
 * and an arg-max policy player, one move for each of B canonical boards (the mover is
 * player 0, what Arena hands a player); one launch, a wave per board. With
 * V = valid_moves(state, 0) under the context's token limit and s0 = get_score(state, 0),
 * the candidate set C of a board is
 *   RANDOM  V;
 *   GREEDY  s_a = get_score(., 0) after make_move(copy, a, 0, deterministic=true) for a in
 *           V, m = max s_a: {a in V : s_a = m} if m > s0, else V & [0,12) if non-empty, else
 *           V & [30,60) if non-empty, else V (the fallback order of :106-111, taken
 *           literally). The reference scores seat 1 after the move; this scores the mover;
 *   POLICY  {a in V : pi[b][a] = max over V of pi[b]} (pi: B x 409 f32, exact equality).
 * The action is the k-th set bit of C in action order, k = floor(u |C|), u = uniform 0 of
 * the Philox stream (seed, board_base + b, (8 << 24) | stream).
 * active (B u8, nullable): rows with 0 are skipped and none of their outputs is written.
 * cand_out (B x 7 u64, packed like spl_valid_moves: C) and best_out (B i32: m for GREEDY,
 * s0 otherwise) are nullable. SPL_EINVAL: NULL ctx / state / action, B < 0, kind outside
 * 0..2, POLICY with NULL pi, stream > 0xFFFFFF. B == 0 launches nothing. */
#define SPL_PLAYER_RANDOM 0
#define SPL_PLAYER_GREEDY 1
#define SPL_PLAYER_POLICY 2
int spl_player_move(const spl_ctx *ctx, int B, const int8_t *state, const uint8_t *active,
                    int kind, const float *pi, uint64_t seed, uint32_t stream,
                    uint32_t board_base, int16_t *action, uint64_t *cand_out,
                    int32_t *best_out, void *hip_stream);

/* SplendorGame.getSymmetries (SplendorGame.py:59-61) -> Board.get_symmetries
 * (SplendorLogicNumba.py:349-395) for E examples (state E x S, pi E x 409 f32, valid E x 7
 * u64). Outputs K = 10 + 2n variant slots per example in the reference's order: identity,
 * 3 tiers x 3 card permutations, then per player up to 2 reserve permutations;
 * present[E][K] = 1 for emitted slots (reserve permutations depend on #reserved cards). */
int spl_symmetries(const spl_ctx *ctx, int E, const int8_t *state, const float *pi,
                   const uint64_t *valid, int8_t *out_state, float *out_pi, uint64_t *out_valid,
                   uint8_t *present, void *hip_stream);

/* Lazy symmetry expansion: the variants are never stored; training rows are produced from
 * the unexpanded examples when a batch is assembled.
 * spl_symmetry_counts: number of variants Board.get_symmetries emits for each of E boards:
 * 10 + sum over players of (0, 0, 1, 2)[#reserved cards] (SplendorLogicNumba.py:349-395).
 * count: E u8. */
int spl_symmetry_counts(const spl_ctx *ctx, int E, const int8_t *state, uint8_t *count,
                        void *hip_stream);

/* M training rows assembled from E unexpanded examples in one launch. Row i is variant number
 * ordinal[i] (0-based, among the variants get_symmetries emits for that board, in its order:
 * the present slots of spl_symmetries) of example example[i]:
 *   x       M x R x 7 f32   the permuted board, cast (what train feeds the network)
 *   pi      M x 409  f32    permuted policy
 *   valid   M x 409  u8     permuted legality, one byte per action (0/1)
 *   winner  M x n    f32,  scdiff  M x n  i32    copied from the example
 * example: M i64, ordinal: M i32 (device). A row with example[i] outside [0, E) or
 * ordinal[i] outside [0, count) reads nothing, is written as zeros and ORs
 * SPL_ERR_BAD_INDEX into *err (nullable). E == 0 or M == 0 launches nothing. */
int spl_gather_examples(const spl_ctx *ctx, int E, int M, const int8_t *state, const float *pi,
                        const uint64_t *valid, const float *winner, const int32_t *scdiff,
                        const int64_t *example, const int32_t *ordinal, float *x, float *out_pi,
                        uint8_t *out_valid, float *out_winner, int32_t *out_scdiff, int32_t *err,
                        void *hip_stream);

/* One fused random-policy self-play step per board (BASELINE config 2; the move loop of
 * Coach.executeEpisode, Coach.py:71-100, with a uniform random policy):
 *   canonical -> valid mask -> action = k-th legal, k = floor(U(seed,b,step,0)*count)
 *   -> make_move(real board, player, chance draws 1,2) -> check_end -> if ended:
 *   games_done[b] += 1 = g and re-init with the deal of game g: draws 0..28 of stream
 *   0x80000000 | g (so deals can be drawn ahead of the game end; steps < 2^31), player=0.
 * games_done is required (it keys the deals). Outputs mask (B x 7), action (B), ended
 * (B x n), all per step. */
int spl_rollout_step(const spl_ctx *ctx, int B, int8_t *state, int8_t *player,
                     uint64_t *mask_out, int16_t *action_out, float *ended_out,
                     int32_t *games_done, uint64_t seed, uint32_t step, uint32_t board_base,
                     void *hip_stream);

/* K consecutive spl_rollout_step calls (steps step0 .. step0+K-1) in one launch: each
 * workgroup keeps its boards on chip for all K moves, so board bytes cross HBM once per
 * launch. Per-move outputs are stacked by move: mask_out [K][B][7] (may be NULL),
 * action_out [K][B], ended_out [K][B][n]; state, player and games_done hold the result
 * after move K. Bit-identical to K spl_rollout_step calls. */
int spl_rollout_run(const spl_ctx *ctx, int B, int K, int8_t *state, int8_t *player,
                    uint64_t *mask_out, int16_t *action_out, float *ended_out,
                    int32_t *games_done, uint64_t seed, uint32_t step0, uint32_t board_base,
                    void *hip_stream);

/* Random playouts to the end of the game, outcomes only: the leaf evaluation of a search
 * player that needs no network (PUCT with uniform priors, splendor/playout.py) and
 * Monte-Carlo outcome estimates of arbitrary positions. Row b of `state` (B x S) is a board
 * whose mover is player[b] (nullable = 0: a canonical MCTS leaf). Each row runs `playouts`
 * (P, 1..64) independent playouts; playout j of row b is task b P + j, with Philox board id
 * board_base + b P + j (uint32 arithmetic). Step t (0-based) of a task is spl_rollout_step's
 * without the re-deal, on stream step0 + t: V = the mover's legality mask under the
 * context's token limit, candidate set C, action = the k-th set bit of C in action order,
 * k = floor(u0 |C|), make_move on the real board with chance uniforms u1 and u2, end check
 * (u0, u1, u2 = uniforms 0, 1, 2 of the stream). C is
 *   UNIFORM    V;
 *   BUY_FIRST  V & {0..11, 27..29} (buy a visible card, buy a reserved card) if non-empty,
 *              else V.
 * A task stops at the first step after which the end vector is non-zero: that vector (seat
 * order of the input board, no roll) is its outcome and steps = t + 1. A task that has not
 * ended after max_steps moves contributes a zero vector, has steps = max_steps and adds 1 to
 * *unfinished (device i32, nullable; the kernel's only global atomic); with max_steps >= 62 n
 * no legal position can be unfinished. The input board is not end-checked before its first
 * move (the caller excludes finished boards, as MCTS does through leaf_valid).
 *   result    B x n f32   the sum of the row's P outcomes in f32, added in ascending j, then
 *                         divided by (float)P (no FMA contraction: one defined value)
 *   steps_out B x P i32   each task's steps (nullable)
 *   pi_out    B x 409 f32 the uniform prior over V of the input board: 1.0f / (float)|V| on
 *                         legal actions, 0 elsewhere (nullable)
 * active (B u8, nullable): rows with 0 run nothing and none of their outputs is written.
 * One launch; boards stay on chip for the whole playout and only the outputs are written to
 * HBM. SPL_EINVAL before any launch: NULL ctx / state / result, B < 0, policy outside 0..1,
 * playouts outside 1..64, max_steps outside 1..1024, step0 + max_steps > 0x80000000 (streams
 * with the top bit set key deals). B == 0 launches nothing. */
#define SPL_PLAYOUT_UNIFORM   0
#define SPL_PLAYOUT_BUY_FIRST 1
int spl_playout(const spl_ctx *ctx, int B, const int8_t *state, const int8_t *player,
                const uint8_t *active, int policy, int playouts, int max_steps,
                uint64_t seed, uint32_t step0, uint32_t board_base,
                float *result, float *pi_out, int32_t *steps_out, int32_t *unfinished,
                void *hip_stream);

/* spl_playout for the search's leaves, safe to capture in a graph: the stream base is read on
 * the device, and the rows may be given as the NN-leaf list. The rows are canonical boards whose
 * mover is seat 0 (spl_playout with player == NULL). Which rows run:
 *   leaf_index and leaf_count both given: the segmented list exactly as spl_mcts_select_compact
 *     writes it and spl_nn_forward_indexed reads it: ceil(B / 64) counts, segment j's entries at
 *     leaf_index[64 j .. 64 j + leaf_count[j]), in any order inside a segment (the counts need no
 *     alignment; a count is read clamped to 0..64 and an entry outside 0..B-1 runs nothing);
 *   else active given: the rows with active[b] != 0;  else: every row.
 * call_seq is one device u32 that the kernel only reads: with c = *call_seq when the kernel
 * runs, the stream base is step0 = (c mod 2^23) SPL_PLAYOUT_SEQ_STREAMS. The caller advances the
 * counter (a stream-ordered add is an ordinary captured operation), so every replay of a
 * captured launch draws new streams. max_steps is limited to 1..SPL_PLAYOUT_SEQ_STREAMS, so
 * consecutive calls' streams never overlap and step0 + max_steps <= 0x80000000 always holds.
 * For every row b that runs, result, pi_out and steps_out equal, bit for bit, those of
 * spl_playout(player = NULL, active = exactly those rows, step0 as above): task keys stay tied
 * to the row, not to the list position (playout j of row b draws from Philox board id
 * board_base + b P + j), and the row's result is the f32 sum in ascending j over (float)P. Rows
 * that do not run keep every output byte; *unfinished accumulates as in spl_playout.
 * With a list a workgroup owns 64 / P consecutive list entries; the grid is sized for B
 * entries, every workgroup finds its entries from a scan of the segment counts, and one past
 * the end of the list leaves before it stages anything. SPL_EINVAL before any launch: NULL ctx /
 * state / result / call_seq, active together with a list, exactly one of leaf_index /
 * leaf_count NULL, B < 0, policy outside 0..1, playouts outside 1..64, max_steps outside
 * 1..256. B == 0 launches nothing. */
#define SPL_PLAYOUT_SEQ_STREAMS 256
int spl_playout_seq(const spl_ctx *ctx, int B, const int8_t *state, const uint8_t *active,
                    const int32_t *leaf_index, const int32_t *leaf_count,
                    int policy, int playouts, int max_steps, uint64_t seed,
                    const uint32_t *call_seq, uint32_t board_base,
                    float *result, float *pi_out, int32_t *steps_out, int32_t *unfinished,
                    void *hip_stream);

/* spl_playout_seq blended into a value buffer (AlphaGo's mixed leaf value): the rows, the task
 * keys (board id board_base + b P + j, stream base from *call_seq) and each row's f32 mean m (the
 * sum in ascending j over (float)P) are spl_playout_seq's; instead of storing m, every row b that
 * runs and every seat i gets
 *   v[b][i] = (1.0f - l) * v[b][i] + l * m[b][i]
 * in f32 exactly as written (two products, one sum, no FMA contraction), read and written in
 * place (v: B x n f32, typically the network's values of the same leaf list). l is *lambda, one
 * device f32 read when the kernel runs and clamped with fminf(fmaxf(x, 0.f), 1.f) (a NaN counts
 * as 0): like call_seq it is a pointer so that a host write reaches every later replay of a
 * captured launch. With l == 0 every workgroup leaves before it stages anything and v is
 * untouched. Rows that do not run keep every byte of v; there is no pi_out and no steps_out (the
 * priors stay the caller's); *unfinished accumulates as in spl_playout. SPL_EINVAL before any
 * launch: as spl_playout_seq, plus NULL lambda or NULL v. B == 0 launches nothing. */
int spl_playout_mix(const spl_ctx *ctx, int B, const int8_t *state, const uint8_t *active,
                    const int32_t *leaf_index, const int32_t *leaf_count,
                    int policy, int playouts, int max_steps, uint64_t seed,
                    const uint32_t *call_seq, uint32_t board_base,
                    const float *lambda, float *v, int32_t *unfinished, void *hip_stream);


/* ===================================================================== MCTS
 * Device-resident batched PUCT search (MCTS.py), one tree per board/game, B trees.
 * The reference's MCTS(game, nnet, args).getActionProb(canonicalBoard, temp=1,
 * force_full_search) (MCTS.py:45-97) maps to:
 *     spl_mcts_set_roots(roots)                 -- re-root (tree persists when keep_tree)
 *     repeat until every tree spent its budget:
 *         spl_mcts_select(leaf_state, leaf_mask, leaf_valid)   -- MCTS.search descent
 *         <network on leaf_state/leaf_mask -> pi[B][409], v[B][n]> (nnet.predict, :138)
 *         spl_mcts_backup(leaf_mask, pi, v)     -- expansion + backup (:134-176)
 *     spl_mcts_root_stats(counts, qsa, probs, q) -- :61-97 (temp = 1)
 * Every tree runs exactly one simulation per select/backup pair, so each tree's search
 * is the reference's sequential search. Trees own device memory allocated at create. */
typedef struct spl_mcts spl_mcts;
typedef struct {
    int num_sims;            /* numMCTSSims (main.py:110) */
    int ratio_full;          /* ratio_fullMCTS: fast search = num_sims / ratio_full */
    double prob_full;        /* prob_fullMCTS: P(full search) (MCTS.py:54) */
    double cpuct;            /* cpuct */
    double fpu;              /* fpu (>0: parent-relative; <=0: absolute) (MCTS.py:203) */
    int forced_playouts;     /* forced playouts + policy-target pruning (MCTS.py:56,69-74) */
    double dirichlet_alpha;  /* > 0 enables root noise at step 0 of full searches */
    double dirichlet_temp;   /* temperature[0]: softmax before noise (MCTS.py:142) */
    int temp_threshold;      /* tempThreshold (Coach.py:82-83), self-play only */
    int node_cap;            /* maximum node slots of one tree (its transposition table and
                                node page table are sized for it) */
    int edge_cap;            /* maximum edge units of one tree (its edge page table). Edges are
                                stored in two tiers of 8-byte units: every edge one unit (prior,
                                action) in its node's run, and an edge with statistics (Nsa,
                                Qsa, child link) 3 more in its node's visit block */
    uint64_t seed;           /* Philox key for search/self-play randomness */
    uint32_t board_base;     /* global id of tree 0 (multi-GPU sharding) */
    int selfplay;            /* 1: trees play games (spl_mcts_reset_games / spl_mcts_commit) */
    int out_cap;             /* self-play: finished-example queue capacity (examples) */
    int node_boards;         /* 1: keep every node's canonical board (8 x rows bytes per node
                                slot), so a descent through linked edges skips the in-tree
                                transition (getNextState, MCTS.py:155-157) — the descent then
                                runs one transition per simulation instead of one per level */
    long long pool_nodes;    /* node slots shared by all B trees (0: B x node_cap) */
    long long pool_edges;    /* edge units shared by all B trees (0: B x edge_cap). Trees draw
                                node pages (64 slots) and edge pages (2048 units) from these
                                pools on demand and return them when garbage is collected, so
                                memory follows the sum of the live trees, not B x the largest */
} spl_mcts_config;

/* The handle takes the context's token limit and rules (spl_ctx_set_rules) as they are at
 * create and keeps them: its trees store legality masks, so a handle never changes rules. */
int spl_mcts_create(const spl_ctx *ctx, int B, const spl_mcts_config *cfg, spl_mcts **out);
int spl_mcts_destroy(spl_mcts *m);
int spl_mcts_rules(const spl_mcts *m);
/* HBM bytes of the whole search arena: the shared node / edge pools, per tree its page
 * tables, transposition table (power of two >= node_cap / 0.7) and path, + self-play buffers. plan_bytes: the same figure before creating it (pool
 * sizing by the caller); device_bytes: of a created arena. */
long long spl_mcts_plan_bytes(const spl_ctx *ctx, int B, const spl_mcts_config *cfg);
long long spl_mcts_device_bytes(const spl_mcts *m);
/* roots: B canonical boards (device). keep_tree: look the root up in the persistent
 * transposition table and keep its subtree (exact GC of unreachable nodes). */
int spl_mcts_set_roots(spl_mcts *m, const int8_t *roots, int keep_tree, int force_full,
                       void *hip_stream);
/* same, for the trees with active[t] != 0 only (active: B u8, device; NULL = all). Inactive
 * trees keep their tree untouched and get no search budget: Arena's per-player MCTS
 * objects (Arena.py:94-160) search only on their own turns. */
int spl_mcts_set_roots_active(spl_mcts *m, const int8_t *roots, const uint8_t *active, int keep_tree,
                              int force_full, void *hip_stream);
/* Arena move choice (the Arena players of Coach.py:152-153: np.argmax(getActionProb(x, temp=0)[0]),
 * MCTS.py:87-92): per active tree, the action with the largest (pruned) root count, ties
 * broken uniformly by Philox (cfg.seed, board_base + t, ST_BEST | stream, draw 0) with
 * ST_BEST = 6 << 24 and stream < 2^24 (the caller's game id base and ply), written to
 * action[t] (B i16, device). */
int spl_mcts_pick_best(spl_mcts *m, const uint8_t *active, uint32_t board_base, uint32_t stream,
                       int16_t *action, void *hip_stream);
/* leaf_state: B x S int8, leaf_mask: B x 7 u64, leaf_valid: B u8 (1 = needs the network) */
int spl_mcts_select(spl_mcts *m, int8_t *leaf_state, uint64_t *leaf_mask, uint8_t *leaf_valid,
                    void *hip_stream);
/* select + the trees whose leaf needs the network listed segment by segment (ABI 11):
 * segment j = trees 64 j .. 64 j + 63; leaf_count (device, ceil(B / 64) i32, 16-byte aligned)
 * holds each segment's number of such trees and leaf_index (device, B i32) their ids at
 * leaf_index[64 j .. 64 j + leaf_count[j]) in no particular order; the list is the segments'
 * entries in segment order. Pair with spl_nn_forward_indexed (or spl_playout_seq) so the
 * network (the playouts) runs on those leaves only (terminal leaves and idle trees need no evaluation: ~30 % of all trees per
 * iteration at BASELINE config 3's steady state). (ABI 10 kept one compact list and one count:
 * every 64-tree workgroup then took its place with a returning atomic on one counter.) */
int spl_mcts_select_compact(spl_mcts *m, int8_t *leaf_state, uint64_t *leaf_mask, uint8_t *leaf_valid,
                            int32_t *leaf_index, int32_t *leaf_count, void *hip_stream);
/* pi: B x 409 f32 (policy over all actions, as predict returns), v: B x n f32 */
int spl_mcts_backup(spl_mcts *m, const uint64_t *leaf_mask, const float *pi, const float *v,
                    void *hip_stream);
/* spl_mcts_backup for the trees whose leaf is of the given kinds only (bit 0: NN leaves, the
 * expansion + backup of MCTS.py:134-176; bit 1: terminal leaves, :125-131 then :169-176).
 * Trees are independent, so a caller may back up the terminal leaves on a second stream
 * while the network evaluates the NN leaves (their backup needs no pi / v: NULL allowed). */
#define SPL_LEAF_NN 1
#define SPL_LEAF_TERMINAL 2
/* kinds | SPL_BACKUP_DEFER_GC (self-play handles, ABI 10): no collection launch for the trees
 * whose simulation was withdrawn (a leaf that did not fit); the caller runs spl_mcts_commit
 * before the next select, and the collection it launches takes them. The self-play driver
 * backs up this way: one k_gc launch per iteration instead of two (~5 us, empty at steady
 * state). Without it, or without a commit before the next select, collect as before. */
#define SPL_BACKUP_DEFER_GC 4
int spl_mcts_backup_kind(spl_mcts *m, const uint64_t *leaf_mask, const float *pi, const float *v, int kinds,
                         void *hip_stream);
/* counts B x 409 i64 (root visit counts Nsa), qsa B x 409 f64 (-42 = unvisited), probs
 * B x 409 f64 (temp = 1), q B x n f64, adjusted B x 409 i64 (counts after policy-target
 * pruning, MCTS.py:69-74; = counts without forced playouts); any may be NULL */
/* ps: B x 409 f32, the root's stored priors Ps (nodes_data[s][2], MCTS.py:147/176: after
 * root Dirichlet noise when it was applied), 0 for illegal actions and for trees without a
 * root. */
int spl_mcts_root_priors(spl_mcts *m, float *ps, void *hip_stream);
int spl_mcts_root_stats(spl_mcts *m, int64_t *counts, double *qsa, double *probs, double *q,
                        int64_t *adjusted, void *hip_stream);
/* Principal variations: a read-only walk of the stored trees, `lines` lines of at most `depth`
 * moves per tree (what the search expects after the move, without re-rooting, which would
 * collect the rest of the tree). Order a node's edges that have a visit record (Nsa >= 1) by
 * (Nsa descending, action ascending): the raw counts, not the forced-playout-pruned ones. Line k
 * (0-based) of tree t starts with the k-th root edge in that order; every level below the root
 * takes the first edge in that order at the node reached through the previous edge's stored
 * link. Entry (t, k, d) of action / visits / q / prior (B x lines x depth each) is that edge's
 * action, Nsa, Qsa and stored prior: Qsa is the f64 as stored, the value for the mover at that
 * node (canonical seat 0 of that node); the prior is the noised one at a root that was noised
 * (what spl_mcts_root_priors returns). After a level is written the walk ends with the first of
 * these that applies, in this order, written to end[t][k] (B x lines u8):
 *   DEPTH      the line is `depth` moves long;
 *   UNLINKED   the last edge's child is not stored / not linked (-1, or a link outside the
 *              node pool, which is never dereferenced);
 *   TERMINAL   the last edge's child is a terminal node;
 *   UNVISITED  the child is expanded but has no edge with Nsa >= 1;
 * and a tree without a root, or with fewer than k + 1 visited root edges, gives NONE. length[t][k]
 * (B x lines i32) is the number of levels written (0 for NONE). The kernel writes every entry:
 * those at and past `length` get action -1, visits 0, q -42.0 (root_stats' unvisited qsa) and
 * prior 0. A line cannot cycle (a child's round is above its parent's); `depth` bounds the walk
 * regardless. One launch, one wave per tree, loads only; valid whenever spl_mcts_root_stats is,
 * and nothing in the handle changes. action and length are required, visits / q / prior / end
 * may be NULL. SPL_EINVAL before any launch: NULL m / action / length, lines outside
 * 1..SPL_PV_MAX_LINES, depth outside 1..SPL_PV_MAX_DEPTH. */
#define SPL_PV_MAX_LINES 16
#define SPL_PV_MAX_DEPTH 64
#define SPL_PV_END_DEPTH     0
#define SPL_PV_END_UNLINKED  1
#define SPL_PV_END_TERMINAL  2
#define SPL_PV_END_UNVISITED 3
#define SPL_PV_END_NONE      4
int spl_mcts_pv(spl_mcts *m, int lines, int depth,
                int16_t *action, int32_t *visits, double *q, float *prior,
                int32_t *length, uint8_t *end, void *hip_stream);
/* ---- self-play (Coach.executeEpisode, Coach.py:50-100), selfplay=1 only ----
 * reset_games: deal B new games (Board.init_game via Philox) and start their searches.
 * commit: for every tree whose search budget is spent, play the move on device:
 *   pi = root visit counts (pruned if forced playouts), record (board, player, pi, valids,
 *   q) if it was a full search, sample the action with temperature 2 before tempThreshold
 *   moves and 0.2 after (Coach.py:19-33, 82-83), getNextState with chance, getGameEnded;
 *   on game end write every example of the game with winner = roll(r, -player) and
 *   score difference (Coach.py:89-98) to the example queue and deal a new game; re-root
 *   the tree at the next canonical board (exact GC) and draw the next search type. */
int spl_mcts_reset_games(spl_mcts *m, void *hip_stream);
/* restart_games: like reset_games for the games with restart[t] != 0 only (restart: B u8,
 * device): each abandons its current game (examples staged for it are discarded; nothing
 * is written to the example queue) and is dealt its next game (game number + 1), with a
 * fresh tree. Call between iterations. Not in the reference (its episodes run one after
 * another): the batched driver uses it to spread B games that started together over the
 * phases of a game (bench warm-up). */
int spl_mcts_restart_games(spl_mcts *m, const uint8_t *restart, void *hip_stream);
int spl_mcts_commit(spl_mcts *m, void *hip_stream);
/* copy up to `max` finished examples to caller buffers (state E x S i8, pi E x 409 f32,
 * valid E x 7 u64, winner E x n f32, scdiff E x n i32, q E x n f32, meta E x 4 i32 =
 * (global board id, game number, example index in game, player)), write the count to
 * *n_out (device int32) and empty the queue (examples beyond `max` are dropped). Any
 * output pointer may be NULL. */
/* out (device, 2 x i32): [0] finished examples waiting in the queue, [1] examples dropped
 * so far because the queue (out_cap) was full when their game ended or a drain asked for
 * fewer than were queued. Self-play arenas only. */
int spl_mcts_counters(spl_mcts *m, int32_t *out, void *hip_stream);
/* out (device, 4 x i32): free node pages, free edge pages, node / edge page requests that
 * found the pool empty so far (each such leaf was withdrawn for collection or counted as
 * unexpanded in its tree's header). pool_pages (host): pages in the node / edge pools and
 * their sizes (node slots / edges per page). */
int spl_mcts_pool_state(spl_mcts *m, int32_t *out, void *hip_stream);
int spl_mcts_pool_pages(const spl_mcts *m, long long *out4);   /* pages, pages, NPG, units/page */
int spl_mcts_drain_examples(spl_mcts *m, int8_t *state, float *pi, uint64_t *valid,
                            float *winner, int32_t *scdiff, float *q, int32_t *meta, int max,
                            int32_t *n_out, void *hip_stream);
/* copies the B per-tree headers (208 bytes each, layout in splendor/mcts.py) to `out` */
int spl_mcts_headers(spl_mcts *m, int32_t *out, void *hip_stream);

/* out B x 4 i32 per tree: node slots used, edge slots used, live nodes (the root and every
 * node whose round exceeds the root's: what garbage collection keeps, MCTS.py:79-85) and
 * their edges. Capacity planning diagnostic (tools/tree_sizes.py). */
int spl_mcts_tree_sizes(spl_mcts *m, int32_t *out, void *hip_stream);

/* predict input conversion (GenericNNetWrapper.py:160-161): int8 boards [B][R][7] -> f32
 * written transposed as x[B][7][R] (SplendorNNet.py:129 layout), packed mask -> bool bytes
 * (valid may be NULL) */
int spl_nn_input(const spl_ctx *ctx, int B, const int8_t *state, const uint64_t *mask,
                 float *x, uint8_t *valid, void *hip_stream);
/* deterministic hash-prior network (see oracle or_fake_predict): parity tests and
 * tree-only throughput runs. spl_hash_eval = mode 0 (spread priors, values in [-1, 1));
 * mode 1: peaked priors, values near +-1 (deep trees like the random-init SplendorNNet's) */
int spl_hash_eval(const spl_ctx *ctx, int B, const int8_t *state, const uint64_t *mask,
                  float *pi, float *v, void *hip_stream);
int spl_hash_eval_mode(const spl_ctx *ctx, int B, const int8_t *state, const uint64_t *mask,
                       float *pi, float *v, int mode, void *hip_stream);

/* ===================================================================== network
 * SplendorNNet inference (SplendorNNet.py:56-159 in eval mode; GenericNNetWrapper.predict
 * :141-168 minus the host round trip) as one fused kernel: int8 boards [B][R][7] + packed
 * masks [B][7] -> pi [B][409] = softmax(masked logits, invalid -> -1e8) and v [B][n] =
 * tanh(value head). f32 arithmetic on bf16 MFMAs, every f32 operand split exactly into three
 * bf16 parts (six products per chunk, the largest in its own f32 accumulator): the per-column
 * layers on v_mfma_f32_32x32x16_bf16, the per-leaf layers on v_mfma_f32_16x16x32_bf16
 * (DESIGN.md §4).
 *
 * packed_weights: spl_nn_packed_floats(n) floats, 16-byte aligned, the eval-mode network
 * with BatchNorms folded (splendor/nnet.py pack_weights). For each of the 13 linear layers
 * (N outputs, K inputs) in the order dense2d_1[0], dense2d_1[3], partialgpool_1 dense,
 * dense2d_3, dense1d_4, partialgpool_4 dense, dense1d_5[0], dense1d_5[3], partialgpool_5
 * dense, output_layers_PI[0], [1], output_layers_V[0], [1]:
 *     Kp = K rounded up to 8; NT = ceil(N / T)
 *     first 4 layers (T = 32, v_mfma_f32_32x32x2_f32, K in 2 halves of S = Kp / 2):
 *         weights [NT][S/4][64][4]: element (nt, q, l, j) = W[32 nt + l % 32][4 q + j + (l / 32) S]
 *     other 9 (T = 16, v_mfma_f32_16x16x4_f32, Kp a multiple of 16, k groups interleaved):
 *         weights [NT][Kp/16][64][4]: element (nt, q, l, j) = W[16 nt + l % 16][16 q + 4 (l / 16) + j]
 *     (0 outside N x K)
 *     bias    [T NT] (0-padded)
 * then the per-board-column BatchNorm affines of dense2d_1 and partialgpool_1:
 * s1[7], t1[7], sp1[7], tp1[7] (y = x * s + t); then, from the next 16-byte boundary, the
 * 13 layers again as exact three-part bf16 splits (w = hi + mid + lo by truncation) for the
 * bf16-MFMA form of those layers: the first 5 (the per-column layers and dense1d_4, whose
 * weights are the A operand of v_mfma_f32_32x32x16_bf16) per layer [4][Kp16/16][3][64][8] bf16 (Kp16 = K rounded
 * up to 16), element (nt, c, p, l, j) = part p of W[32 nt + l % 32 - o][16 c + 8 (l / 32) + j]
 * (o = 8 for partialgpool_1, whose outputs follow its 8 pooled channels, else 0; 0 outside),
 * two bf16 per float slot; then the other 8 layers the same way for 16x16x32: per layer
 * [NT16][Kp32/32][3][64][8] bf16 (NT16 = ceil(N / 16), Kp32 = K rounded up to 32), element
 * (nt, c, p, l, j) = part p of W[16 nt + l % 16][32 c + 8 (l / 16) + j]. The f32 copies of the
 * 13 layers stay in the layout (the biases are read from them). Returns the float count or
 * SPL_EINVAL. */
int spl_nn_packed_floats(int n_players);
int spl_nn_forward(int n_players, int B, const int8_t *leaf_state, const uint64_t *leaf_mask,
                   const float *packed_weights, float *pi, float *v, void *hip_stream);
/* the same network on the rows listed by leaf_index / leaf_count only, in the segmented form
 * spl_mcts_select_compact writes (B = the number of trees: ceil(B / 64) segment counts,
 * leaf_count 16-byte aligned): boards, masks and outputs of row r = every listed leaf_index
 * entry; other rows of pi / v are left untouched. */
int spl_nn_forward_indexed(int n_players, int B, const int8_t *leaf_state, const uint64_t *leaf_mask,
                           const int32_t *leaf_index, const int32_t *leaf_count, const float *packed_weights,
                           float *pi, float *v, void *hip_stream);
/* Opt-in reduced-precision modes of the same kernel. precision = the number P of leading bf16
 * parts (hi, mid, lo by truncation) of every matrix-product operand that enter the MFMAs:
 *
 *     mode  name            P   products per chunk                     weight parts read
 *     0     SPL_NN_F32      3   six (hh, hm, mh, hl, lh, mm)           hi, mid, lo
 *     1     SPL_NN_BF16X2   2   hh, hm, mh                             hi, mid
 *     2     SPL_NN_BF16     1   hh                                     hi
 *
 * (dense2d_1's int8 boards are exact in one part: P weight-part products there.) Truncation
 * applies only where an operand enters an MFMA; accumulators, biases, BatchNorm affines, ReLU,
 * pooling, the masked softmax and tanh stay f32 on each layer's untruncated outputs. The packed
 * weights are the same in every mode; parts that are not multiplied are not read. Relative
 * operand error: 2^-16 (BF16X2), 2^-8 (BF16). Reduced modes change search trees: they are for
 * self-play data generation and the arena, not for parity checks.
 * leaf_index == NULL and leaf_count == NULL: rows 0 .. B as spl_nn_forward; both non-NULL: the
 * segmented list of spl_nn_forward_indexed; exactly one NULL, or a precision outside 0 .. 2:
 * SPL_EINVAL before any launch. spl_nn_forward and spl_nn_forward_indexed are SPL_NN_F32. */
#define SPL_NN_F32 0
#define SPL_NN_BF16X2 1
#define SPL_NN_BF16 2
int spl_nn_forward_mode(int n_players, int B, const int8_t *leaf_state, const uint64_t *leaf_mask,
                        const int32_t *leaf_index, const int32_t *leaf_count,
                        const float *packed_weights, float *pi, float *v, int precision,
                        void *hip_stream);

/* ---- staged leaves: the mask kernel hands the network its tiles ----
 * The mask kernel that runs before the network has every leaf board on chip and knows which
 * leaves need the network; with a staged leaf buffer it writes them where the network kernel
 * wants them — list order, 32-leaf tiles, each tile already the int8 image the kernel keeps in
 * LDS — so a network tile starts with one round of contiguous 16-byte loads instead of a scan
 * of the segment counts, two dependent index hops and a byte scatter.
 *
 * The buffer: spl_nn_stage_bytes(n_players, B) bytes of device memory, 16-byte aligned,
 * allocated and ZERO-FILLED ONCE by the caller (never again: the fill only gives the bytes the
 * kernels never write a defined value). Layout (byte offsets; a16(x) = x rounded up to 16):
 *     0                       i32   total: the number of listed leaves; 12 bytes reserved
 *     16                      i32   rows[B]: the tree row of list entry p
 *     M = a16(16 + 4 B)       u64   mask[B][7]: the legality masks in list order
 *     X = a16(M + 56 B)       i8    x[ceil(B / 32)][7][32][X0S]: tile p / 32, slot p % 32 holds
 *                                   entry p's board transposed, x[.][c][p % 32][r] = board[r][c],
 *                                   X0S = R rounded up to 8, plus 4 if that is an even number of
 *                                   dwords (60 / 76 / 92 for 2 / 3 / 4 players)
 * The list is spl_mcts_select_compact's: segments of 64 trees in order, trees ascending inside
 * a segment. Entries at and past `total` (rows, masks, tile slots) keep what they last held;
 * the network kernel neither stores results for them nor lets them reach a result (bytes r >= R of
 * a slot stay zero and meet zero weights). Returns the size or SPL_EINVAL. */
long long spl_nn_stage_bytes(int n_players, int B);
/* spl_mcts_select whose mask kernel also fills `stage` (leaf_mask by tree row, leaf_state and
 * leaf_valid are written exactly as by spl_mcts_select). leaf_valid must be 16-byte aligned:
 * every 64-tree segment counts the listed leaves of the segments before it from those bytes. */
int spl_mcts_select_staged(spl_mcts *m, int8_t *leaf_state, uint64_t *leaf_mask, uint8_t *leaf_valid,
                           void *stage, void *hip_stream);
/* The same mask-and-stage kernel on caller-supplied canonical boards without a tree: for the B
 * boards of leaf_state, the rows with leaf_valid[b] != 0 get their mask (leaf_mask[b], under
 * the context's token limit and rules) and are staged. B == 0 launches nothing. */
int spl_nn_stage_leaves(const spl_ctx *ctx, int B, const int8_t *leaf_state, const uint8_t *leaf_valid,
                        uint64_t *leaf_mask, void *stage, void *hip_stream);
/* The network on the staged leaves: pi / v rows rows[p] for p < total are written, all others
 * left untouched; bit-identical to spl_nn_forward_mode on the same list. B = the number of
 * trees the buffer was sized and filled for. precision as spl_nn_forward_mode.
 * All three: NULL or misaligned arguments (stage, leaf_valid, packed_weights: 16 bytes), or a
 * precision outside 0 .. 2, return SPL_EINVAL before any launch. */
int spl_nn_forward_staged(int n_players, int B, const void *stage, const float *packed_weights,
                          float *pi, float *v, int precision, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
