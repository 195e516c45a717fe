/*
 * azsp.h -- C ABI of the MI355X batched self-play engine (libazsp.so).
 *
 * The upstream reference (michaelnny/alpha_zero) is pure Python and has no FFI; the "plugin API"
 * of its self-play hot path is three Python call surfaces.  This header is what a binding for
 * that path would bind (ctypes stub in INTEGRATION.md); each entry point names the reference
 * interface it replaces (paths relative to the reference repo):
 *
 *   azsp_create / azsp_destroy        engine for G concurrent games: replaces one actor process per game
 *                                     (alpha_zero/training_go.py:317-347, core/pipeline.py:166-218)
 *   azsp_reset_games                  env.reset() for every slot                (envs/base.py:93-112, envs/go.py:76-86)
 *   azsp_env_step                     BoardGameEnv.step / legal_actions / observation / score as a batch
 *                                     (envs/go.py:88-161, envs/gomoku.py:45-83, envs/go_engine.py:417-441,
 *                                      :123-152, envs/base.py:228-259)
 *   azsp_set_state                    the `env` argument of uct_search()        (core/mcts_v2.py:301-311)
 *   azsp_begin_move                   add_dirichlet_noise at the start of a search (core/mcts_v2.py:375-376, :565-566)
 *   azsp_set_states                   the `env` arguments of G uct_search() calls at once: every slot loads, keeps or drops its
 *                                     position from device tensors in one launch (core/mcts_v2.py:301-311)
 *   azsp_begin_moves                  add_dirichlet_noise and the `warm_up` argument per slot (core/mcts_v2.py:375-376)
 *   azsp_read_searches                the tuples G uct_search() calls return, into device tensors (core/mcts_v2.py:450)
 *   azsp_select                       Phase 1 of (parallel_)uct_search: best_child descents, virtual loss,
 *                                     and env.observation() of the leaves       (core/mcts_v2.py:572-611)
 *   azsp_expand_backup                Phases 2-3: expand + backup, then (when the budget is met) policy,
 *                                     move, sample recording, env.step, re-root (core/mcts_v2.py:614-657,
 *                                      core/pipeline.py:323-346)
 *   azsp_round                        azsp_expand_backup + azsp_select in one launch
 *   azsp_get_status / azsp_get_search the tuple uct_search() returns            (core/mcts_v2.py:450)
 *   azsp_commit_move                  sub-tree reuse after the caller chose the move (core/mcts_v2.py:436-446)
 *   azsp_dropin_step                  one iteration of uct_search's simulation loop around the caller's eval_func: expand + backup of the
 *                                     evaluated leaves, selection of the next ones, and everything eval_func needs, in ONE host round trip
 *                                     (core/mcts_v2.py:378-421, :568-625)
 *   azsp_harvest                      data_queue.put((game_seq, stats))         (core/pipeline.py:283, :349-380)
 *   azsp_set_actor_state              per-game re-read of var_resign_threshold / checkpoint tag (core/pipeline.py:232-246)
 *   azsp_set_budgets                  no counterpart in the reference: opt-in.  num_simulations per game slot
 *   azsp_set_playout_cap              no counterpart in the reference: opt-in.  A random fraction of an actor's moves gets the full
 *                                     search, the others a cheap one; azsp_harvest_search_class tells the samples apart
 *   azsp_set_leaf_symmetry            no counterpart in the reference (it transforms in the learner only, core/pipeline.py:636-643):
 *                                     opt-in.  Every leaf position reaches the evaluator under a board symmetry, chosen at random or
 *                                     fixed, and its priors are mapped back before the node is expanded; azsp_leaf_symmetries tells a
 *                                     caller which one each feature row was written under
 *   azsp_set_forced_playouts          no counterpart in the reference: opt-in.  Forced playouts at the root with policy-target pruning
 *                                     (KataGo, Wu 2019, 3.2); azsp_read_target_policies hands a drop-in caller the pruned targets
 *   azsp_set_gumbel                   no counterpart in the reference: opt-in.  Gumbel root search (Danihelka et al. 2022): sequential
 *                                     halving at the root and the completed-Q policy target; azsp_read_gumbel_moves hands a drop-in
 *                                     caller the move
 *   azsp_set_fpu                      no counterpart in the reference: opt-in.  First-play urgency reduction (Leela Zero, KataGo): what an
 *                                     unvisited child is worth in the PUCT selection
 *   azsp_replay_gather                UniformReplay.sample + batch tensors + random transformation (core/replay.py:72-83,
 *                                      core/pipeline.py:636-643)
 *   azsp_dihedral                     apply_horizontal_flip / apply_vertical_flip / apply_rotation
 *                                     (utils/transformation.py:34-110)
 *   azsp_bias_act                     BatchNorm + residual add + ReLU after each convolution (core/network.py:42-82)
 *   azsp_conv3x3_tiled                a whole conv3x3 + BatchNorm (+ skip) + ReLU of a ResNetBlock (core/network.py:42-82)
 *   azsp_resblock_tiled               a whole ResNetBlock of a 64-filter tower in one launch (intermediate activation in LDS)
 *   azsp_tile_layout / azsp_tiled_bytes the tower's resident activation layout
 *   azsp_conv3x3_split                the same layer at the reference's fp32 precision class (core/pipeline.py:91-123 evaluates
 *                                     in fp32): values as hi + lo f16 pairs, three f16 MFMA products, fp32 accumulation
 *   azsp_split_layout / azsp_split_bytes the split-precision tower's activation layout
 *   azsp_split_features / azsp_stem_split / azsp_head_split   the stem and both heads of the same fp32-class evaluator
 *                                     (core/network.py:101-156)
 *   azsp_*_tiled_f16 / azsp_fc_heads_f16  the bf16 evaluator entries with f16 activations and weights
 *
 * Conventions: every function returns 0 on success or a negative AZSP_E* code; the message is
 * available from azsp_last_error().  No exceptions and no callbacks cross this boundary.  Pointers
 * named *_dev are device (HBM) addresses owned by the caller (e.g. torch tensors) and must stay
 * alive until `stream` (a hipStream_t, NULL = default stream) has drained; pointers named *_host
 * are host memory.  One host thread per engine.  Colours at this boundary use the reference's
 * ids: Go black = 1, white = -1; Gomoku black = 1, white = 2 (envs/go.py:63-64, envs/base.py:33-34).
 */
#ifndef AZSP_H
#define AZSP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AZSP_GAME_GO 0
#define AZSP_GAME_GOMOKU 1

#define AZSP_FEAT_I8 0
#define AZSP_FEAT_F32 1
#define AZSP_FEAT_BF16 2
#define AZSP_FEAT_F16 3
#define AZSP_FEAT_BF16_TILED 4 /* bf16 in the evaluator's tiled layout, 2K+1 planes (K = num_stack) padded to 32 channels (azsp_stem_tiled) */
#define AZSP_FEAT_F16_TILED 5  /* the same layout with f16 elements (azsp_stem_tiled_f16) */
#define AZSP_FEAT_F16_SPLIT 6  /* the input of the fp32-class evaluator's stem (azsp_stem_split): split layout [row][plane: hi, lo][4 chunks]
                                  [N*N][8] f16 with 32 channels, azsp_split_bytes(rows, N, 32) bytes; the planes are 0 / 1 = exact f16 values,
                                  so only the hi plane is ever written (the caller zero-initialises the tensor once) */

#define AZSP_OK 0
#define AZSP_EINVAL (-1)   /* bad argument / unsupported configuration */
#define AZSP_ENOMEM (-2)
#define AZSP_EDEVICE (-3)  /* HIP runtime error */
#define AZSP_EENGINE (-4)  /* engine-side fault flag raised (node pool, depth, staging), see azsp_last_error */

/* Game status codes reported by azsp_get_status */
#define AZSP_ST_NEED_ROOT 0
#define AZSP_ST_SEARCH 1
#define AZSP_ST_MOVE_DONE 2
#define AZSP_ST_IDLE 3
#define AZSP_ST_WAIT_BUF 4

typedef struct AzspConfig {
    int32_t game;              /* AZSP_GAME_* */
    int32_t board_size;        /* Go: 5, 9, 13, 19   Gomoku: 7, 9, 13, 15 */
    int32_t num_games;         /* G: concurrent games (one wavefront each) */
    int32_t num_parallel;      /* P: leaves per game per round; 1 selects uct_search semantics (pipeline.py:132-156) */
    int32_t num_simulations;   /* budget: root.N < sims (+P when P > 1)      (mcts_v2.py:378, :568) */
    int32_t max_nodes;         /* node pool per game; 0 = sims + 3P + 8 */
    int32_t root_noise;        /* mcts_v2.py:375 */
    int32_t deterministic;     /* mcts_v2.py:427-429 */
    int32_t reuse_tree;        /* 0: root_node=None on every move (pipeline.py:836) */
    int32_t warm_up_steps;     /* pipeline.py:320 */
    int32_t has_resign;        /* Go only */
    int32_t check_resign_after_steps;
    int32_t force_resign_disabled; /* -1: draw per game with disable_resign_ratio (pipeline.py:244-246); 0/1: fixed */
    int32_t inject_random;     /* 1: noise / uniforms come from azsp_set_injection (parity runs) */
    int32_t inject_moves;      /* plies covered by the injection tables */
    int32_t stop_after_move;   /* 1: drop-in uct_search mode, the caller picks and commits the move */
    int32_t max_plies;         /* >0: a game idles after this many moves (tests) */
    int32_t stop_at_game_end;  /* 1: slots idle after their first game (tests) */
    int32_t feature_dtype;     /* AZSP_FEAT_* of the tensor written by azsp_select */
    int32_t log_moves;         /* keep per-move pi / child_N / Q logs (tests, drop-in mode) */
    int32_t log_capacity;      /* plies per game kept in the log */
    int32_t max_steps;         /* Go: 0 = 2*N*N (go.py:48) */
    int32_t num_to_win;        /* Gomoku (gomoku.py:26) */
    int32_t training_steps;    /* tag copied into every finished game (pipeline.py:271) */
    int32_t rank;              /* added to seed, mirrors set_seed(seed + rank) (pipeline.py:193) */
    int32_t device;            /* HIP device ordinal */
    float c_puct_base;         /* used by the caller to build the pb_c table (azsp_set_tables) */
    float c_puct_init;
    float disable_resign_ratio;
    int32_t num_stack;         /* K = history boards per observation, 1..8 (base.py:228-266): 2K+1 planes [X_t, Y_t, ..., X_t-K+1,
                                  Y_t-K+1, C]; 0 = 8 (callers that predate the field pass 0); > 8 is AZSP_EINVAL */
    double dirichlet_eps;      /* 0.25 (mcts_v2.py:235) */
    double dirichlet_alpha;    /* 0.03 */
    double resign_threshold;   /* <= -1 disables resignation (pipeline.py:216) */
    double komi;               /* 7.5 (go.py:46) */
    uint64_t seed;
} AzspConfig;

/* Sizes the caller needs to allocate its tensors. */
typedef struct AzspGeometry {
    int32_t num_actions;       /* A = N*N (+1 pass for Go) */
    int32_t num_points;        /* N*N */
    int32_t planes;            /* 2 * num_stack + 1 (17 at the default K = 8) */
    int32_t batch_rows;        /* G*P rows of features / priors / values */
    int32_t max_nodes;
    int32_t budget;
    int32_t table_len;         /* entries expected by azsp_set_tables */
    int32_t stage_capacity;    /* max samples per game */
    int64_t device_bytes;      /* HBM allocated by the engine */
    int32_t node_record_bytes;
    int32_t reserved;
} AzspGeometry;

int azsp_create(const AzspConfig* cfg, void** out_engine);
int azsp_destroy(void* engine);
const char* azsp_last_error(void* engine);
int azsp_geometry(void* engine, AzspGeometry* out);

/* pb_c(n) = log((1 + n + base)/base) + init for n = 0..len-1, as the reference evaluates it for a
 * node whose visit count is an np.float32 (pbc_np) or a Python float (fresh root, pbc_py), and
 * float32(sqrt(n)) (mcts_v2.py:99-102).  Host pointers; copied. */
int azsp_set_tables(void* engine, const double* pbc_np_host, const double* pbc_py_host, const float* sqrt32_host, int32_t len);

/* Injected randomness for parity runs: noise[G][moves][A] (np.random.dirichlet outputs) and
 * uniforms[G][moves][16] (the u of each np.random.choice draw).  Host pointers; copied. */
int azsp_set_injection(void* engine, const double* noise_host, const double* uniforms_host, int32_t moves);

/* Start a new game in every slot (env.reset()). */
int azsp_reset_games(void* engine, void* stream);

/* Standalone environment kernels.  actions_dev[G]: action, -1 = resign (Go), -2 = no-op (export only).
 * Outputs (each may be NULL): board int8[G][N*N] (reference colour ids), legal int8[G][A],
 * scalars int32[G][AZSP_ENV_COUNT] (columns below), obs int8[G][2K+1][N][N] (K = num_stack). */
enum {
    AZSP_ENV_KO,          /* the ko point, -1 = none */
    AZSP_ENV_CAPS_BLACK,
    AZSP_ENV_CAPS_WHITE,
    AZSP_ENV_STEPS,
    AZSP_ENV_TO_PLAY,     /* ref id */
    AZSP_ENV_DONE,
    AZSP_ENV_REWARD,
    AZSP_ENV_WINNER,      /* ref id, 0 none */
    AZSP_ENV_AREA_BLACK,  /* Go only, else 0 */
    AZSP_ENV_AREA_WHITE,
    AZSP_ENV_ILLEGAL,     /* 0 = the action was applied; 1 game over, 2 invalid action, 3 illegal action */
    AZSP_ENV_LAST_PASS,
    AZSP_ENV_COUNT
};
int azsp_env_step(void* engine, const int32_t* actions_dev, int8_t* board_dev, int8_t* legal_dev, int32_t* scalars_dev,
                  int8_t* obs_dev, void* stream);

/* Load an arbitrary position into slot `slot` and make it the (fresh, unevaluated) search root.
 * board_host int8[N*N] and hist_host int8[8][N*N] (newest first, hist[0] == board) use reference colour ids; with num_stack K < 8
 * the rows K..7 are ignored (the observation never shows them). */
int azsp_set_state(void* engine, int32_t slot, const int8_t* board_host, const int8_t* hist_host, int32_t to_play,
                   int32_t steps, int32_t ko, int32_t last_was_pass, int32_t caps_black, int32_t caps_white, void* stream);

/* Drop-in mode: hand the Dirichlet draw of this search to the engine (noise_host double[G][A] or NULL) and the
 * `warm_up` flag of uct_search (1: temperature 1.0, 0: temperature 0.1, -1: derive from env.steps <= warm_up_steps). */
int azsp_begin_move(void* engine, const double* noise_host, int32_t warm_up, void* stream);

/* Batched form of azsp_set_state: ONE launch in which the wave of every slot reads its own row of the caller's DEVICE tensors (no
 * host packing, no copy, no synchronisation).  boards_dev int8[G][N*N] and hist_dev int8[G][hist_boards][N*N] (newest first, 1 <=
 * hist_boards <= 8; the engine's history rows beyond hist_boards become empty boards) use reference colour ids; pos_dev
 * int32[G][AZSP_PS_COUNT] holds the columns below; result_dev int32[G] receives one AZSP_SS_* code per slot.  A slot whose action
 * is AZSP_PSA_LOAD ends in exactly the state azsp_set_state leaves it in (a fresh, unevaluated search root); AZSP_PSA_KEEP leaves the
 * slot untouched (tree, status, history, noise state); AZSP_PSA_IDLE frees its tree and sets its status to AZSP_ST_IDLE.  A LOAD row
 * that is refused (AZSP_SS_INVALID, AZSP_SS_GAME_OVER; any other action value is INVALID too) leaves the slot idle as well; the
 * engine's fault flags are not touched.  (Plain #defines, not an enum: these are columns of a tensor the CALLER fills.) */
#define AZSP_PS_ACTION 0      /* AZSP_PSA_* */
#define AZSP_PS_TO_PLAY 1     /* ref id */
#define AZSP_PS_STEPS 2
#define AZSP_PS_KO 3          /* the ko point, -1 = none */
#define AZSP_PS_LAST_PASS 4   /* 1: the last move was a pass */
#define AZSP_PS_CAPS_BLACK 5
#define AZSP_PS_CAPS_WHITE 6
#define AZSP_PS_COUNT 7
#define AZSP_PSA_KEEP 0
#define AZSP_PSA_LOAD 1
#define AZSP_PSA_IDLE 2
#define AZSP_SS_OK 0
#define AZSP_SS_INVALID 1     /* to_play is no colour id; negative (or over-wide) steps / captures; a ko point off the board, on a stone, or given at Gomoku */
#define AZSP_SS_GAME_OVER 2   /* Go: steps >= max_steps; Gomoku: the board is full */
int azsp_set_states(void* engine, const int8_t* boards_dev, const int8_t* hist_dev, int32_t hist_boards, const int32_t* pos_dev,
                    int32_t* result_dev, void* stream);

/* Batched form of azsp_begin_move (drop-in mode): noise_dev double[G][A] on the DEVICE or NULL, warm_dev int32[G] with one `warm_up`
 * flag per slot (1 / 0 as azsp_begin_move, -1 = derive from env.steps) or AZSP_BM_SKIP = leave the slot alone: its noise row is not
 * read and the state of a search it has pending is unchanged.  Each slot's wave copies its own noise row.  Does not synchronise. */
#define AZSP_BM_SKIP (-2)
int azsp_begin_moves(void* engine, const double* noise_dev, const int32_t* warm_dev, void* stream);

/* Batched form of azsp_get_search + azsp_get_status into DEVICE tensors: pi_dev double[G][A], child_n_dev float[G][A] = the last
 * finished search of every slot, q_dev double[G][AZSP_STQ_COUNT] and status_dev int32[G][AZSP_STC_COUNT] as azsp_get_status.  Each
 * may be NULL.  The log slot it reads is the one the slot's search writes: in drop-in mode (log_moves = 0) log slot 0 of every game,
 * i.e. azsp_get_search(slot, 0); with log_moves the slot of the game's current ply, min(ply, log_capacity - 1), which holds the
 * search that has just finished while the status is AZSP_ST_MOVE_DONE.  Does not synchronise. */
int azsp_read_searches(void* engine, double* pi_dev, float* child_n_dev, double* q_dev, int32_t* status_dev, void* stream);

int azsp_select(void* engine, void* features_dev, uint8_t* valid_dev, void* stream);
int azsp_expand_backup(void* engine, const float* priors_dev, const float* values_dev, void* stream);
/* The same two phases for the games [g0, g1) only (g0 % 32 == 0; the tensors are the full-batch ones, indexed by game as above).
 * Games never interact during a search (mcts_v2.py:568-625 runs per game), so disjoint ranges in any order are the whole batch,
 * bit for bit (tested).  EXPERIMENTAL: no product path calls these two entries -- SelfPlayActor runs whole-batch rounds on ONE
 * stream.  They exist for the half-batch overlap experiment (tools/overlap_actor.py; DESIGN "Two streams": measured +0.3 %, not
 * adopted).  The ENGINE kernels of disjoint ranges are exact on two streams; two evaluator FORWARDS in flight at the same time
 * are a separate matter, see DESIGN before putting two forwards on one device. */
int azsp_select_range(void* engine, void* features_dev, uint8_t* valid_dev, int32_t g0, int32_t g1, void* stream);
int azsp_expand_backup_range(void* engine, const float* priors_dev, const float* values_dev, int32_t g0, int32_t g1, void* stream);
int azsp_round(void* engine, const float* priors_dev, const float* values_dev, void* features_dev, uint8_t* valid_dev,
               void* stream);

/* status_host int32[G][AZSP_STC_COUNT] and q_host double[G][AZSP_STQ_COUNT] (columns below; the Q pair is that of the last
 * finished search).  Synchronises the stream. */
enum {
    AZSP_STC_STATUS,  /* AZSP_ST_* */
    AZSP_STC_PLY,
    AZSP_STC_ROOT_N,
    AZSP_STC_N_LEAVES,
    AZSP_STC_LAST_MOVE,
    AZSP_STC_GAMES_DONE,
    AZSP_STC_ROOT_EVAL_PENDING,
    AZSP_STC_NOISE_PENDING,
    AZSP_STC_COUNT
};
enum { AZSP_STQ_ROOT_Q, AZSP_STQ_CHILD_Q /* of the chosen move, 0 without a child node */, AZSP_STQ_COUNT };
int azsp_get_status(void* engine, int32_t* status_host, double* q_host, void* stream);

/* Search outputs of `slot` at log index `ply` (log_moves or drop-in mode): pi double[A], child_N float[A],
 * q double[AZSP_SQ_COUNT] (columns below).  Synchronises the stream. */
enum { AZSP_SQ_ROOT_Q, AZSP_SQ_CHILD_Q /* of the chosen move, 0 without a child node */, AZSP_SQ_ROOT_N, AZSP_SQ_MOVE, AZSP_SQ_COUNT };
int azsp_get_search(void* engine, int32_t slot, int32_t ply, double* pi_host, float* child_n_host, double* q_host, void* stream);

/* Drop-in mode: the caller's chosen moves (int32[G], host); re-roots each tree on the chosen child. */
int azsp_commit_move(void* engine, const int32_t* moves_host, void* stream);

/* Drop-in mode: one iteration of the simulation loop of uct_search / parallel_uct_search (core/mcts_v2.py:378-421, :568-625) around the
 * caller's eval_func in ONE kernel launch and ONE stream synchronisation (the separate entries above cost four launches and eight
 * synchronisations).  priors_host float[rows][A] / values_host float[rows] (rows = G * P) = eval_func's outputs for the leaves of the
 * previous call; both NULL on the first call of a search (nothing to back up yet).  The game's wave runs expand / backup (and the
 * end-of-search work when the budget is met), selects the next leaves into features_dev / valid_dev, and writes status_host
 * int32[G][AZSP_STC_COUNT], q_host double[G][AZSP_STQ_COUNT] (as azsp_get_status; q_host may be NULL), valid_host uint8[rows] and the first features_bytes bytes of
 * features_dev (the observation planes eval_func receives; 0 = none; feature_dtype must be a plain [rows][2K+1][N][N] tensor: I8 / F32 /
 * BF16 / F16) -- through a page-locked staging buffer of the engine that the kernel reads and writes directly, so no copy command is
 * issued.  priors_dev / values_dev are the caller's evaluator tensors (unused by this entry beyond validation; azsp_expand_backup
 * reads them).  Host pointers may be pageable. */
int azsp_dropin_step(void* engine, const float* priors_host, const float* values_host, float* priors_dev, float* values_dev,
                     void* features_dev, uint8_t* valid_dev, int32_t* status_host, double* q_host, uint8_t* valid_host, void* features_host,
                     int64_t features_bytes, void* stream);

/* Collect finished games.  states int8[cap][2K+1][N][N] (K = num_stack), pi float[cap][A], z float[cap] receive the samples of
 * whole games back to back; games_host int32[max_games][AZSP_GR_COUNT] (columns below).  Synchronises the stream. */
enum {
    AZSP_GR_START,            /* first sample row of the game */
    AZSP_GR_LENGTH,           /* number of samples */
    AZSP_GR_WINNER,           /* ref id, 0 none */
    AZSP_GR_AREA_BLACK,
    AZSP_GR_AREA_WHITE,
    AZSP_GR_PASSES,
    AZSP_GR_RESIGNED,
    AZSP_GR_RESIGN_DISABLED,
    AZSP_GR_MARKED,           /* marked for resign */
    AZSP_GR_COULD_WON,
    AZSP_GR_MARKED_PLAYER,    /* ref id, 0 none */
    AZSP_GR_UID,
    AZSP_GR_TRAINING_STEPS,   /* tag of the weights that STARTED the game */
    AZSP_GR_REWARD,
    AZSP_GR_LAST_PLAYER,      /* ref id */
    AZSP_GR_SLOT,             /* game slot; a caller that merges the rows of several engines tags it with its rank (below) */
    AZSP_GR_COUNT
};
#define AZSP_GR_SLOT_RANK_SHIFT 20 /* merged rows: slot | rank << AZSP_GR_SLOT_RANK_SHIFT (alpha_zero_amd/core/gather.py) */
#define AZSP_GR_SLOT_MASK ((1 << AZSP_GR_SLOT_RANK_SHIFT) - 1)
int azsp_harvest(void* engine, int8_t* states_dev, float* pi_dev, float* z_dev, int32_t sample_capacity,
                 int32_t* games_host, int32_t max_games, int32_t* n_samples_out, int32_t* n_games_out, void* stream);

/* Diagnostics: the production random streams (no injection) of every game slot for plies 0 .. plies-1 of its current game,
 * drawn exactly as the search draws them and without changing any state: noise_host double[G][plies][A] = the Dirichlet(alpha)
 * vectors add_dirichlet_noise uses (core/mcts_v2.py:259-260: one draw over all A actions), unif_host double[G][plies][tries] =
 * the uniforms behind np.random.choice (core/mcts_v2.py:434; try t is consumed only if try t-1 was rejected).  Counter-based
 * Philox4x32-10 keyed by (seed + rank, slot, game uid, ply, action / try): statistical tests in tests/ use this entry. */
int azsp_rng_probe(void* engine, int32_t plies, int32_t tries, double* noise_host, double* unif_host, void* stream);

/* Optional second output of azsp_harvest: moves_dev int16[sample_capacity] receives, for every harvested sample, the move
 * that was played from its position (a flat action index, board_size^2 = pass, -1 = the mover resigned) -- what the
 * reference's env.history / to_sgf() holds for a self-play game (envs/base.py:224-226, core/pipeline.py:276-281).
 * NULL (the default) disables it.  The buffer must stay valid for every later azsp_harvest call. */
int azsp_harvest_moves(void* engine, int16_t* moves_dev);

/* Third optional output of azsp_harvest: extra_host int32[max_games][AZSP_GX_COUNT] (host memory, row i belongs to games_host
 * row i; columns below).  games_host column AZSP_GR_TRAINING_STEPS is the tag of the weights that STARTED the game, which is what the
 * reference actor writes (core/pipeline.py:237 -> :271).  NULL (default) disables it. */
enum {
    AZSP_GX_TS_END,        /* training_steps of the weights in use when the game ENDED */
    AZSP_GX_THRESHOLD_LO,  /* the game's own resign threshold: low / high word of its double */
    AZSP_GX_THRESHOLD_HI,
    AZSP_GX_STRADDLED,     /* 1 if the game straddled a weight hot-swap (end tag != start tag) */
    AZSP_GX_COUNT
};
int azsp_harvest_extra(void* engine, int32_t* extra_host);

/* Per-game actor state: the reference actor re-reads the shared resign threshold (core/pipeline.py:241-242) and the weights'
 * training_steps (core/pipeline.py:232-239) before EVERY game.  Both values take effect for games that start after this call
 * (each game keeps the threshold / tag it started with; resign_disabled is drawn per game only while the threshold is > -1,
 * core/pipeline.py:244-246).  resign_threshold <= -1 disables resignation (the learner's warm-up value, core/pipeline.py:449-459). */
int azsp_set_actor_state(void* engine, double resign_threshold, int32_t training_steps);

/* Per-game simulation budgets (no counterpart in the reference: opt-in).  budgets_dev int32[G]: the simulations per move of every
 * slot, 0 = the engine's num_simulations.  The node pool and the pb_c tables are sized from num_simulations, so that is the upper
 * limit: the kernel clamps a value into [1, num_simulations] (callers refuse out-of-range values before the upload).  A slot's search
 * ends when its root has budget (+ num_parallel in parallel mode) visits, the rule azsp_create applies to num_simulations
 * (core/mcts_v2.py:378 / :568).  Values are sticky until the next call; a game that is mid-search uses the new value at its next
 * budget check.  One launch over all slots, nothing is synchronised. */
int azsp_set_budgets(void* engine, const int32_t* budgets_dev, void* stream);

/* Playout-cap randomisation for actor mode (no counterpart in the reference: opt-in, off by default).  At the start of every move a
 * game draws one uniform u from its own Philox stream (key seed + rank; counters slot, game uid, (ply << 12) | 0xFFE, 0x2000 -- a
 * counter word neither the Dirichlet nor the move-sampling stream uses).  u < full_prob: a FULL move -- the slot's budget, root noise
 * as configured.  Otherwise a FAST move -- fast_simulations (+ num_parallel), no root noise.  The tree is reused across both kinds as
 * reuse_tree says; warm-up temperature, resignation and everything else are untouched.  Fast moves are recorded like full ones (game
 * length, moves and sample rows keep meaning the whole game); the class travels with the sample (azsp_harvest_search_class).
 * fast_simulations == 0 turns the cap off.  AZSP_EINVAL in drop-in mode (stop_after_move), for fast_simulations outside
 * 0..num_simulations and for full_prob outside [0, 1].  Takes effect for the moves that start after this call.  (As with
 * num_simulations = 1, fast_simulations = 1 at num_parallel = 1 leaves a fresh root without a visited child to play.) */
int azsp_set_playout_cap(void* engine, int32_t fast_simulations, double full_prob);

/* Optional output of azsp_harvest next to azsp_harvest_moves (no counterpart in the reference: opt-in): class_dev
 * uint8[sample_capacity] receives 1 for every harvested sample whose move was a full search and 0 for a fast move of the playout
 * cap; with the cap off every byte is 1.  NULL (the default) disables it.  The buffer must stay valid for every later harvest. */
int azsp_harvest_search_class(void* engine, uint8_t* class_dev);

/* Leaf symmetry (no counterpart in the reference search: opt-in, off by default).  With op the symmetry of a feature row, D_op the
 * transform of azsp_dihedral (out[c][i][j] = in[c][src_op(i, j)]; on a policy row the N*N board entries move the same way, the pass
 * column stays) and inv(op) its inverse (3 <-> 5, every other op is its own):
 *   - azsp_select / azsp_round / azsp_dropin_step write D_op(observation) into the row, in every feature_dtype layout;
 *   - when the row's node is expanded it stores D_inv(op)(priors row), from priors_dev and from the priors_host of azsp_dropin_step;
 *   - the value is used as it is.
 * Nothing else sees the op: recorded samples, azsp_env_step observations, harvests and logs stay in the true orientation.  A search
 * with op k around an evaluator E is, bit for bit, the plain search around "transform by k, run E, map the priors back".
 * mode: AZSP_SYM_OFF (the default), AZSP_SYM_RANDOM, or 0..7 = that op for every row; anything else is AZSP_EINVAL.  It holds for the
 * rows selected after the call; a row in flight keeps the op it was written with.  AZSP_SYM_RANDOM draws op = floor(8 u) per written
 * row, the root-evaluation row included, from a Philox stream of its own: key seed + rank; counters slot, the slot's count of rows
 * written under a mode other than AZSP_SYM_OFF since azsp_create, 0xFFD, 0x3000 -- a counter word no other stream uses.  The count
 * advances in drop-in mode too, so repeated searches of one slot see fresh ops.  (Plain #defines, not an enum: mode is an argument.) */
#define AZSP_SYM_OFF (-1)
#define AZSP_SYM_RANDOM (-2)
int azsp_set_leaf_symmetry(void* engine, int32_t mode);
/* ops_dev uint8[G * num_parallel]: the op each feature row of the last select was written with -- 0 for a row that select did not
 * write, and everywhere with the mode off.  What a host callback needs to undo or account for the transform.  Does not synchronise. */
int azsp_leaf_symmetries(void* engine, uint8_t* ops_dev, void* stream);

/* Forced playouts at the root with policy-target pruning (KataGo, Wu 2019, 3.2; no counterpart in the reference search: opt-in, off by
 * default).  k >= 0, finite (0 = off, KataGo uses 2); anything else is AZSP_EINVAL.  Valid in actor and drop-in mode; holds for the
 * selections and move ends after the call.  The rule applies at the root only, to every search whose move is not a fast move of the
 * playout cap, with or without root noise.  N(a), W(a) = the root's child row, P(a) = the prior the root's PUCT term uses (the float64
 * noisy prior at a noisy root, else the float32 prior converted to double), legal(a) = the mask the selection applies.
 *   Forcing (select).  Virtual loss touches W only, so the descents in flight are counted: v(a) = the leaves already accepted into the
 *   current leaf batch whose path starts with root move a (duplicates count; terminal hits are backed up, not in flight),
 *   n_eff(a) = N(a) + v(a), T_eff = sum_a N(a) + leaves of the batch.  A legal child is forced when n_eff > 0 and
 *   (double)n_eff * (double)n_eff < (k * (double)P(a)) * (double)T_eff, evaluated as written (no square root).  If any child is forced
 *   the root's arg-max returns the forced child with the lowest action index, else what it returns without the rule.  Nothing else of
 *   the descent changes.
 *   Pruning (end of the move; no virtual loss is outstanding).  T = sum_a N(a); c* = the first legal action with the largest N;
 *   score(a, m) = the -q + u the root's selection evaluates for child a with N(a) replaced by m in u (q stays W(a) / N(a); pb_c, the
 *   square-root entry and float64 / float32 as at the root's final visit count); S* = score(c*, N(c*)).  For every legal a != c* with
 *   N(a) > 0: f(a) = the largest integer with f^2 <= (k * (double)P(a)) * (double)T; m runs from N(a) - 1 down to max(N(a) - f(a), 0)
 *   and stops at the first m with score(a, m) >= S*; N'(a) = the last m that passed (N(a) if none); a child reduced to a single playout
 *   is pruned outright (N' = 0).  N'(c*) = N(c*); without a visited child nothing is pruned.  The policy target is the search policy
 *   (same temperature exponent, float64 for Go, float32 pairwise sum for Gomoku) of N' instead of N.
 * What uses which: the move is chosen from the unpruned policy, and the move log, azsp_get_search and azsp_read_searches keep
 * reporting the unpruned search; the pi row staged for the sample -- everything azsp_harvest hands out -- and the slot's target row
 * are the pruned target.  prune_target = 0 forces without pruning: the target is the plain policy.  A fast move of the playout cap is
 * neither forced nor pruned.  With k = 0 neither phase evaluates the rule (what stays is a flag per select launch and per descent) and
 * every output is what it is without this call.
 * Every finite k is accepted, however large: only min(f(a), N(a)) enters the pruning, so its cost per child is bounded by N(a), and a
 * k beyond any N^2 / (P T) simply forces every visited child with P > 0 and lets every such child be pruned down to 0.  The first call
 * with k > 0 allocates the target rows on the engine's device and, like azsp_create, leaves that device selected on the calling thread. */
int azsp_set_forced_playouts(void* engine, double k, int32_t prune_target);
/* pi_dev float64[G][A]: per slot the policy target of its most recent search that finished with forced playouts on (k > 0) -- what a
 * drop-in caller records instead of the pi of azsp_read_searches.  A row is zero before the slot's first such search; with pruning off
 * it equals the plain policy.  AZSP_EINVAL before forced playouts were enabled for the first time (the rows are allocated by that
 * call, never by a launch).  Does not synchronise. */
int azsp_read_target_policies(void* engine, double* pi_dev, void* stream);

/* Gumbel root search: sequential halving over Gumbel-sampled root actions and a completed-Q policy target (Danihelka et al., ICLR 2022,
 * "Policy improvement by planning with Gumbel"; no counterpart in the reference search: opt-in, off by default).  Below the root the
 * search stays PUCT, unchanged.  m = the most root actions considered (0 = off; < 0 is AZSP_EINVAL), c_visit and c_scale finite and
 * >= 0 (the paper uses 50 and 1.0), else AZSP_EINVAL.  Valid in actor and drop-in mode.  m holds for the moves that begin after the
 * call: a move is classed when its root is ready (first evaluated, or kept by a commit), and it keeps its class and its m -- Gumbel or
 * plain, with or without Dirichlet noise -- until it ends, whatever is set meanwhile (AZSP_STC_NOISE_PENDING reads 2 while a Gumbel base
 * row is due, 1 while Dirichlet noise is); c_visit and c_scale are read when they are used.  AZSP_EINVAL while forced playouts are on, and azsp_set_forced_playouts(k > 0) is AZSP_EINVAL while this is on.
 *   Quantities at the root of slot g.  n0(a) = N(a) of the root's children when the search begins (non-zero only with reuse_tree);
 *   n(a) = N(a) - n0(a) + v(a), v(a) = the leaves of the current batch whose path starts with a; t = sum_a n(a);
 *   n_sched = max(1, S - rootN_begin), S = the slot's simulations for this move, rootN_begin = the root's visit count when the search
 *   begins; m' = min(m, number of legal actions) -- pass is legal wherever the selection admits it.
 *   Considered-visit sequence cv(t; m', n_sched), integer arithmetic, t unbounded.  If m' <= 1: t.  Else L = ceil(log2 m'), k = m',
 *   base = 0, and repeat: e = max(1, n_sched div (L k)); if t < e k return base + t div k; else t -= e k, base += e,
 *   k = max(2, k div 2).
 *   Base row.  b(a) = g(a) + log(max((double)P(a), 1e-45)): g(a) = the slot's Gumbel(0, 1) draw for this search, P(a) = the root's
 *   float32 prior.  Formed once per search where the Dirichlet noise is added otherwise, which is not applied in this mode (root_noise
 *   is ignored).  g(a) = -log(-log u) from the engine's counter-based stream; with injection (azsp_set_injection) the `noise` table
 *   carries g(a) instead of Dirichlet vectors, and in drop-in mode the noise row of azsp_begin_move[s] does (a row never handed over
 *   reads as it was left: zero at first, which makes the search the deterministic one on the priors).
 *   Values, float64, evaluated as written.  q(a) = -W(a) / N(a) from the root's row as it stands (kept visits and virtual losses
 *   included); T = sum_legal N(a); v_root = root_W / root_N; v_mix = (v_root + T * (sum_{N(a)>0} P(a) q(a) / sum_{N(a)>0} P(a))) / (1 + T),
 *   v_root when no child is visited (or their priors sum to 0); cq(a) = q(a) if N(a) > 0 else v_mix;
 *   sigma(a) = ((c_visit + max_legal N) * c_scale) * ((cq(a) + 1) / 2); score(a) = b(a) + sigma(a).  The two prior-weighted sums are
 *   added in no fixed order: scores are defined up to that rounding.
 *   Root selection, in front of every descent.  Among the legal actions with n(a) == cv(t) the largest score, ties to the lowest
 *   index; if no action has that count, the largest score among the legal actions with the smallest n(a).
 *   End of the move.  a* = the largest score among the legal actions with the largest N(a) - n0(a), ties to the lowest index; in a
 *   search that made no simulation (a kept sub-tree that already holds the budget: every N(a) - n0(a) is 0) only children with
 *   N(a) > 0 are candidates if there is one, so that the move has a child node, as a sampled move always has.  In actor
 *   mode it is the move, whatever warm_up_steps and `deterministic` say; azsp_read_gumbel_moves hands it to a drop-in caller.
 *   pi'(a) = softmax over the legal a of log(max(P(a), 1e-45)) + sigma(a), the maximum subtracted first, 0 for illegal a.
 * What uses which: pi' is the slot's target row (azsp_read_target_policies) and the pi row staged for the sample; the move log,
 * azsp_get_search and azsp_read_searches keep the plain visit policy, child N and Q.  A fast move of the playout cap runs the plain
 * search: its target row is the plain policy and it has no a* (-1).  With m = 0 nothing of this is evaluated and every output is what it
 * is without this call.  While m > 0 the noise rows of azsp_rng_probe are the g(a) the searches draw.  The first call with m > 0
 * allocates the n0 rows, and the target rows unless forced playouts already have, on the engine's device and leaves it selected.
 * The effect on playing strength is a training experiment; it has not been measured. */
int azsp_set_gumbel(void* engine, int32_t m, double c_visit, double c_scale);
/* move_dev int32[G]: a* of each slot's most recent finished Gumbel root search, -1 before the first and after a fast move -- the move
 * a drop-in caller commits.  AZSP_EINVAL before the mode was enabled for the first time.  Does not synchronise. */
int azsp_read_gumbel_moves(void* engine, int32_t* move_dev, void* stream);

/* First-play urgency reduction (Leela Zero; KataGo's fpuReductionMax = 0.2, rootFpuReductionMax = 0.1; no counterpart in the reference:
 * opt-in, off by default).  The reference scores an unvisited child with Q = 0, a draw (mcts_v2.py:99-109: -q + u with q = W / max(N, 1)).
 * With the rule on, the selection at a node i whose mover chooses among the legal actions a is, expression for expression:
 *   Q_self(i)  = W(i) / N(i), the node's own statistics as they are stored when the selection runs (its parent's row; the root's own
 *                slots for the root; virtual losses of descents in flight included), 0 if N(i) = 0 -- Tree.Q(i) of the reference's
 *                arithmetic: a float64 quotient of two Python floats on a freshly created root, a float32 quotient of two np.float32
 *                everywhere else (a re-used root, every node below the root);
 *   mass(i)    = sum of (double)P(i, a) over the actions a < A with N(i, a) > 0, P being the prior the u term of that node uses (the
 *                float64 row at a root with Dirichlet noise, else the float32 prior), accumulated in float64 in this order: lane l of 64
 *                adds its own elements a = l, l + 64, l + 128, ... in ascending order to 0.0, then the 64 partial sums are combined by the
 *                butterfly v[l] = v[l] + v[l ^ o] for o = 32, 16, 8, 4, 2, 1;
 *   fpu(i)     = (double)Q_self(i) - r * sqrt(mass(i)) in float64, r = r_root at the root of the search, r = r_tree below it;
 *   a child with N(i, a) > 0 is scored as it is without the rule;
 *   a child with N(i, a) = 0 takes fpu(i) - W(i, a) in place of -q: at a root with Dirichlet noise (the float64 scores)
 *                (fpu - (double)W) + u in float64; everywhere else ((float)fpu - W) + u in float32, fpu rounded to float32 once.
 *                W(i, a) of an unvisited child is the number of descents in flight through it (virtual loss touches W only), so a leaf that
 *                is being evaluated keeps repelling the next descent of its batch.
 * The u term, the legal mask, the first-maximum tie-break and lazy child creation are untouched.  (0, 0) is a valid setting -- an
 * unvisited child is then worth its parent's value -- and is not off: off is on = 0, with which every expression is the reference's.
 * Forced playouts: the forced child is still tested in front of the arg-max, and the pruning of the policy target scores visited
 * children only.  Gumbel root search: the root's choice and the completed-Q target are unchanged, the rule holds below the root with
 * r_tree.  Playout cap: fast moves follow the rule too.  Nothing else is touched: pi, child_N, Q, samples and targets are produced by
 * the same code from another search.
 * r_tree, r_root: finite and >= 0, else AZSP_EINVAL (also with on = 0).  Holds for the selections launched after the call, those of a
 * search in progress included.  An engine that has had the rule on launches the select kernel that holds it for the rest of its life
 * (DESIGN 7.12).  The effect on playing strength is a training experiment; it has not been measured. */
int azsp_set_fpu(void* engine, int32_t on, double r_tree, double r_root);

/* Auxiliary training targets per sample (KataGo, Wu 2019, 4.1; no counterpart in the reference actor: opt-in, off by default).  With the
 * feature on, actor mode stages next to every sample what the engine computes anyway and otherwise drops:
 *   root value: the search's own value estimate root_Q of the sample's move, the value azsp_get_search reports in AZSP_SQ_ROOT_Q
 *     (a Python float on a fresh root, an np.float32 quotient on a kept sub-tree), stored as float.  It is the mover's view already.
 *   owner boards of the game's FINAL position, once per game: ob = black | (rb & ~rw), ow = white | (rw & ~rb), rb / rw = the empty
 *     points reachable through empty points from a black / white stone -- the two sets whose sizes are AZSP_GR_AREA_BLACK / _WHITE
 *     (Tromp-Taylor area, no dead-stone removal: envs/go_engine.py:123-152).  Go, every kind of game end: two passes and max_steps score
 *     that position anyway; a resignation leaves the board as it was, so its owner boards are those of the position at the
 *     resignation, while AZSP_GR_AREA_* stay 0 for that game as they always did.  Gomoku: ob / ow are the stones of the final board.
 * azsp_harvest_aux hands them out in the mover's perspective, s = +1 for a sample whose mover is black, -1 for white (the bit that
 * selects the colour plane of the state):
 *   ownership int8[cap][N*N]: s * (bit(ob, p) - bit(ow, p)): +1 the mover's point, -1 the opponent's, 0 nobody's;
 *   score float[cap]: Go: s * (float)((double)|ob| - ((double)|ow| + komi)), go_finish's expression (envs/go_engine.py:509-516), so for a
 *     game ended by score it is area black - area white - komi seen by the mover; Gomoku: the sample's z;
 *   root_q float[cap]: the staged root value, unchanged.
 * on != 0: the first such call allocates the staging rows on the engine's device (and leaves it selected, like
 * azsp_set_forced_playouts).  Holds for the moves recorded and the games finished after the call; what was staged earlier, or with the
 * feature off again, reads 0.  Actor mode only: AZSP_EINVAL with stop_after_move.  states, pi, z, the game rows, the move log,
 * azsp_get_search and every other output are what they are without this call.  The effect on playing strength is a training
 * experiment; it has not been measured. */
int azsp_set_aux_targets(void* engine, int32_t on);
/* Optional outputs of azsp_harvest next to azsp_harvest_moves: ownership_dev int8[sample_capacity][N*N], score_dev and root_q_dev
 * float[sample_capacity] as defined above; each may be NULL (the default) on its own.  AZSP_EINVAL (any non-NULL) before the feature was
 * enabled for the first time.  Buffers must stay valid for every later harvest. */
int azsp_harvest_aux(void* engine, int8_t* ownership_dev, float* score_dev, float* root_q_dev);

/* Policy surprise weighting (KataGo, Wu 2019, "Policy Surprise Weighting"; no counterpart in the reference actor: opt-in, off by default):
 * how often each sample of a game is written into the training data follows how much its search's policy target disagrees with the
 * network's own prior, while the number of rows per game stays what it was.  With the feature on, actor mode stages next to every sample
 *   surprise = (float) max(KL, 0),  KL = sum over a with pi(a) > 0 of pi(a) (log pi(a) - log max((double)P(a), 1e-45)) + (Z > 0 ? log Z : 0),
 * in float64, where pi is the float64 row the sample records (the plain policy at its temperature, the pruned target of forced playouts or
 * the Gumbel pi': the surprise is measured on the target the learner is trained towards -- after warm-up the reference's sharpened
 * policy), P the root's prior row as the evaluator returned it (float32, unmasked, before Dirichlet noise) and Z the sum of (double)P(a)
 * over the actions legal at the root.  The sums are wave reductions; their order is not part of the contract.
 * azsp_harvest computes the weights of every game it hands out from the game's staged rows k = 0 .. len - 1:
 *   full_k = 1 unless row k was a fast move of the playout cap (all 1 with the cap off);  part_k = full_k or include_fast;
 *   Nf = sum of full_k;  S = sum over k ascending with part_k of (double)surprise_k  (sequential, in row order);
 *   w_k = S > 0 ? (1 - frac) full_k + (part_k ? frac Nf (double)surprise_k / S : 0) : full_k;   weight_k = (float)w_k,
 * float64 in exactly this operation order.  The weights of a game sum to Nf up to rounding; frac = 0 gives weight == full; a game without
 * surprise is weighted uniformly.  With include_fast a fast move whose cheap search found something the prior did not see earns a place.
 * on != 0: the first such call allocates the staging row on the engine's device (and leaves it selected, like azsp_set_aux_targets).
 * `on` holds for the moves recorded after the call (what was staged earlier, or with the feature off again, reads 0); frac and
 * include_fast hold for the harvests after the call.  Actor mode only: AZSP_EINVAL with stop_after_move, and for frac outside [0, 1].
 * states, pi, z, the game rows, the move log, azsp_get_search and every other output are what they are without this call.  The effect on
 * playing strength is a training experiment; it has not been measured. */
int azsp_set_policy_surprise(void* engine, int32_t on, double frac, int32_t include_fast);
/* Optional outputs of azsp_harvest next to azsp_harvest_moves: surprise_dev and weight_dev float[sample_capacity] as defined above; each may
 * be NULL (the default) on its own.  AZSP_EINVAL (any non-NULL) before the feature was enabled for the first time.  Buffers must stay
 * valid for every later harvest. */
int azsp_harvest_surprise(void* engine, float* surprise_dev, float* weight_dev);

/* Decided-game visit reduction (KataGo's reduceVisits / reducedVisitsMin / reducedVisitsWeight; no counterpart in the reference actor:
 * opt-in, off by default): once one and the same side has clearly led in the last `lookback` searches of a game, the remaining moves are
 * searched with fewer simulations and their samples carry less weight.  Unlike resignation the game goes on and keeps recording.
 * azsp_set_visit_reduction(engine, lookback L, threshold t, min_simulations m, min_weight w):
 *   L = 0 turns the rule off.  AZSP_EINVAL outside 0 <= L <= 8, 0 <= t < 1, 1 <= m <= num_simulations, 0 <= w <= 1, for a NaN, for a
 *   drop-in engine (stop_after_move), as azsp_set_playout_cap, and for L > 0 on an engine with num_simulations > 32767.  The call holds
 *   for the moves that start after it.
 * 1. History.  Every finished search of a batched-actor game pushes b = (mover is Black) ? rq : -rq onto the slot's ring, rq = the double
 *    the move log holds as AZSP_SQ_ROOT_Q -- full and fast moves alike, a Gumbel root too.  The ring has 8 entries, newest first; the
 *    push happens in front of the move choice.  `seen` counts the pushes; a new game and a call that turns the rule on (L > 0 after
 *    L = 0 or after no call) set it to 0.  A call that changes L while the rule is on keeps ring and seen: L is read when it is used.
 * 2. At the start of a move, after the playout cap's class draw (untouched; this rule has no randomness and no Philox word):
 *      seen < L: prop = 0;  else lo = min, hi = max of the newest L entries,  d = lo > 0 ? lo : (hi < 0 ? -hi : 0),
 *      prop = d > t ? (d - t) / (1 - t) : 0;  prop > 1: prop = 1.      float64 in this operation order, no FMA contraction.
 * 3. Budget.  full = the slot's simulations of a full move (azsp_set_budgets or the engine's, clamped into [1, num_simulations]),
 *    m' = min(m, full).  A full-class move searches s = full - (int)(prop * (double)(full - m')) simulations (the cast truncates), + P
 *    in parallel mode as ever; a fast move keeps its fast simulations.  Everything else about the move is what it would be at a slot
 *    budget of s: root noise as configured, forced playouts and pruning on, the Gumbel schedule built from s.  A kept sub-tree whose
 *    root already holds the budget's visits owes no simulation.
 * 4. Base weight.  Every recorded sample stages base = (float)(1 - prop * (1 - w)) with the prop of its own move (fast moves too) and
 *    the w in force when it is recorded.  The staging row and the slot state are allocated by the first call with L > 0 on the engine's
 *    device (which it leaves selected), never by a launch; from then on a move recorded with the rule off, or one that was in progress
 *    when the rule was turned on, stages 1.0f.
 * 5. Harvest.  With fb_k = (double)base_k * full_k the weights of azsp_set_policy_surprise become
 *      Nf = sum fb_k;  S = sum over k ascending with part_k of (double)base_k * (double)surprise_k;
 *      w_k = S > 0 ? (1 - frac) fb_k + (part_k ? frac Nf ((double)base_k * (double)surprise_k) / S : 0) : fb_k;  weight_k = (float)w_k,
 *    sequential in row order.  With policy surprise off (frac = 0, every surprise 0) weight_k = base_k * full_k; with every base 1.0 the
 *    weights are the bits they are without this rule.
 * 6. counters_host[14] counts the moves started with s < full.
 * With the rule never turned on, every output of the engine is the bytes it was.  Playing strength is a training experiment; it has not
 * been measured. */
int azsp_set_visit_reduction(void* engine, int32_t lookback, double threshold, int32_t min_simulations, double min_weight);
/* azsp_harvest_surprise with a third optional output, base_dev float[sample_capacity]: the staged base weight of every row.  It sets all
 * three registrations.  AZSP_EINVAL for surprise_dev before policy surprise was first enabled, for base_dev before the visit reduction
 * was, and for weight_dev before either (with only one of them ever on, the other's values are surprise 0 / base 1).  Buffers must stay
 * valid for every later harvest. */
int azsp_harvest_weights(void* engine, float* surprise_dev, float* weight_dev, float* base_dev);

/* counters_host uint64[16]: simulations, best_child calls, backup edges, leaves, duplicate leaves, terminal hits,
 * moves, games, root evaluations, nodes created, game-rounds, buffer stalls, speculative record prefetches of the select phase,
 * how many of them were used, and the moves started with a reduced budget (azsp_set_visit_reduction). */
int azsp_counters(void* engine, uint64_t* counters_host, int32_t reset, void* stream);

/* Dihedral-8 transform of a batch (no engine needed): op 0 identity, 1 h-flip, 2 v-flip, 3/4/5 = rot90/180/270
 * counter-clockwise (the reference's five), 6 transpose, 7 anti-transpose.  elem_size in bytes (1, 2, 4 or 8).
 * states [B][C][N][N], pi [B][A] with A == N*N or N*N+1 (pass column untouched). */
int azsp_dihedral(const void* states_in_dev, void* states_out_dev, int32_t state_elem_size, const void* pi_in_dev,
                  void* pi_out_dev, int32_t pi_elem_size, int32_t batch, int32_t channels, int32_t board_size,
                  int32_t num_actions, int32_t op, void* stream);

/* Fused convolution epilogue for the leaf evaluator (core/network.py ResNetBlock, network.py:42-82 in eval mode with
 * BatchNorm folded): y[r][c] = act(y[r][c] + bias[c] (+ residual[r][c])) in place, one pass over HBM instead of the
 * separate bias / residual-add / ReLU kernels.  y, residual: [rows][channels] (channels-last activations), dtype
 * AZSP_FEAT_F32 / _BF16 / _F16, channels % 8 == 0; accumulation in fp32, one rounding. */
int azsp_bias_act(void* y_dev, const void* bias_dev, const void* residual_dev, int64_t rows, int32_t channels, int32_t dtype,
                  int32_t relu, void* stream);

/* The residual tower's resident activation layout ("tiled"): [tile = T boards][C/8 channel chunks][T*S*S positions][8 ch]
 * bf16 with T = max(1, 256 / (S*S)) boards per tile (3 at 9x9, 1 from 13x13 up), azsp_tiled_bytes(boards, S, C) bytes.  A tile is what one workgroup of azsp_conv3x3_tiled multiplies at a time:
 * its LDS image equals its global image (flat LDS-DMA copy), fragment reads are conflict-free with immediate k offsets,
 * and the epilogue stores 512 contiguous bytes per instruction.  azsp_tile_layout converts channels-last rows
 * [boards][S][S][C] to (to_tiled = 1) / from (0) that layout at tower entry / exit.  Positions of boards past `boards`
 * in the last tile are never read into a valid output. */
int64_t azsp_tiled_bytes(int64_t boards, int32_t board_size, int32_t channels);
int azsp_tile_layout(const void* src_dev, void* dst_dev, int64_t boards, int32_t board_size, int32_t channels, int32_t to_tiled,
                     void* stream);
/* Fused 3x3 convolution of the residual tower (core/network.py:42-82, eval mode, BatchNorm folded) on the tiled layout:
 * y = act(conv3x3(x, w) + bias [+ residual]); x, residual, y tiled bf16, w_packed [9 taps (ky*3+kx)][C out][C in] bf16, bias
 * float[C].  Weight-stationary MFMA kernels, the filter bank stays in the registers of persistent workgroups.  On the device:
 * (S, C) = (9, 128) 9x9 Go, (17, 64) the 13x13 Gomoku tower, (9, 64) 9x9 Go with 64 filters, (19, 256) the jumbo Go tower (two launches per convolution, the
 * partial sum lives in y: x and residual must not alias y); AZSP_EINVAL for other shapes. */
int azsp_conv3x3_tiled(const void* x_dev, const void* w_packed_dev, const float* bias_dev, const void* residual_dev, void* y_dev,
                       int64_t boards, int32_t board_size, int32_t channels, int32_t relu, void* stream);

/* One whole ResNetBlock (core/network.py:42-82: conv3x3 + BN + ReLU + conv3x3 + BN, + skip, ReLU; eval mode, BatchNorm folded) of a
 * 64-filter tower in ONE launch on the tiled layout: y = relu(conv3x3(relu(conv3x3(x, w1) + b1), w2) + b2 + x).  The intermediate
 * activation stays in LDS and the skip is taken from the input tile already resident there, so a block moves two tensor passes
 * through HBM instead of five; results are bit-identical to two azsp_conv3x3_tiled calls (same MFMA order, same two bf16 roundings).
 * w1 / w2 packed [9 taps][64 out][64 in] bf16, b1 / b2 float[64]; y may alias x.  On the device: (S, C) = (17, 64) the 13x13 Gomoku
 * tower, (9, 64) the 9x9 Go tower with 64 filters (logs/go/9x9_12b64); AZSP_EINVAL for other shapes. */
int azsp_resblock_tiled(const void* x_dev, const void* w1_packed_dev, const float* bias1_dev, const void* w2_packed_dev, const float* bias2_dev,
                        void* y_dev, int64_t boards, int32_t board_size, int32_t channels, void* stream);

/* The residual tower at the reference's precision class (core/network.py:42-82 evaluated in fp32 by core/pipeline.py:91-123).
 * gfx950 multiplies fp32 matrices at 1/16 of its f16 rate and has no TF32, so here an fp32 value v travels as two f16 numbers,
 * hi = f16(v) and lo = f16((v - hi) * 2048), and a product is three f16 MFMAs (w_hi x_hi; w_hi x_lo + w_lo x_hi scaled by 1/2048)
 * accumulated in fp32: 22-bit significands, per-product error <= 3 * 2^-22, i.e. fp32 round-off class (bounded against fp64 next to
 * the library's fp32 convolution in tests/test_split_tower.py).  RANGE: a value beyond f16's finite range (|v| > 65504) cannot be
 * split; it is clamped to +-65504 where the reference's fp32 network would carry it on.  That never happens silently: every kernel
 * that splits values records such an event in a sticky device-side RANGE RECORD (below; the convolution epilogues look at the value
 * IN FRONT of the ReLU -- a pre-activation below -65504 counts although the ReLU zeroes it: deliberately conservative, it costs no
 * instruction and a tower whose negative pre-activations leave the range is about to lose its positive ones; BatchNorm-folded AlphaZero towers stay far
 * inside the range -- activations of the shipped networks peak at ~1e2 -- and alpha_zero_amd.core.network.InferenceNet rescales a
 * network's activations by an exact power of two when a calibration pass finds them near the limit).
 * "Split layout": [board][plane: hi, lo][C/8 channel chunks][S*S positions][8 ch] f16 = azsp_split_bytes(boards, S, C) bytes;
 * azsp_split_layout converts fp32 channels-last rows [boards][S][S][C] to (to_split = 1) / from (0) it.
 * azsp_conv3x3_split: y = act(conv3x3(x, w) + bias [+ residual]); x, residual, y in the split layout; x must not alias y; residual
 * may alias y at 9x9 and must NOT at 17x17 (AZSP_EINVAL: the half-board tiles repeat 15 positions per board in later column tiles);
 * w_split [2 planes: hi, lo][9 taps (ky*3+kx)][C out][C in] f16 with lo = (w - hi) * 2048, bias float[C].  On the device:
 * weight-stationary kernels for (S, C) = (9, 128), (9, 64) and (17, 64) (the 13x13 Gomoku tower behind its pad-3 stem,
 * network.py:101-105; half-board tiles, az_conv_sp17.h); since round 6 every other plane size 3 <= S <= 64 with C = 64, 128 or 256
 * on the wave-per-tile kernel (az_conv_spg.h: e.g. the 19x19 x 256 jumbo tower at the reference's own precision,
 * alpha_zero/training_go_jumbo.py:46-47) -- and the three shapes above too when the call is small (azsp_small_batch_waves below;
 * bit-identical results).  (9, 128) runs PAIRS of boards per workgroup (az_conv_sp2p.h); an odd last board always runs the wave-per-tile
 * kernel, also with that limit at 0 (bit-identical results).  AZSP_EINVAL for other shapes.
 * range_rec_dev: the caller's range record -- two zero-initialised uint32 words in device memory, owned by the caller (one per
 * network: two evaluators in one process never see each other's events), read with azsp_split_range_read; NULL selects the library's
 * per-device default record (azsp_split_range_status). */
int64_t azsp_split_bytes(int64_t boards, int32_t board_size, int32_t channels);
int azsp_split_layout(const void* src_dev, void* dst_dev, int64_t boards, int32_t board_size, int32_t channels, int32_t to_split,
                      uint32_t* range_rec_dev, void* stream);
int azsp_conv3x3_split(const void* x_dev, const void* w_split_dev, const float* bias_dev, const void* residual_dev, void* y_dev,
                       int64_t boards, int32_t board_size, int32_t channels, int32_t relu, uint32_t* range_rec_dev, void* stream);

/* One whole ResNetBlock (core/network.py:42-82: conv3x3 + BN + ReLU + conv3x3 + BN, + skip, ReLU; eval mode, BatchNorm folded) at the
 * reference's precision class in ONE launch on the split layout: y = relu(conv3x3(relu(conv3x3(x, w1) + b1), w2) + b2 + x).  The
 * intermediate activation stays in LDS (half-board tiles, the halo row of each half recomputed), so a block moves two tensor passes
 * through HBM instead of five; results are bit-identical to two azsp_conv3x3_split calls (same MFMA order, same roundings).  w1 / w2 in
 * the packing of azsp_conv3x3_split, b1 / b2 float[64]; y must NOT alias x.  On the device: (S, C) = (17, 64), the 13x13 Gomoku tower
 * (half-board tiles, az_resblock_sp17.h), and (9, 64), the reference's 64-filter 9x9 Go towers (logs/go/9x9_12b64; two boards per tile, an odd
 * last board runs as two wave-per-tile launches); AZSP_EINVAL for other shapes.  range_rec_dev as above. */
int azsp_resblock_split(const void* x_dev, const void* w1_split_dev, const float* bias1_dev, const void* w2_split_dev, const float* bias2_dev,
                        void* y_dev, int64_t boards, int32_t board_size, int32_t channels, uint32_t* range_rec_dev, void* stream);

/* The rest of the fp32-class evaluator on the split layout (core/network.py:101-156):
 * azsp_split_features: observation planes [boards][in_channels <= 32][S][S] fp32 (the engine's AZSP_FEAT_F32 features) -> split
 *   layout with 32 channels (the missing ones zero), azsp_split_bytes(boards, S, 32) bytes.  Not needed when the engine writes its
 *   features with feature_dtype = AZSP_FEAT_F16_SPLIT: that tensor IS the stem's input (what SelfPlayActor does).
 * azsp_stem_split: the stem convolution + BatchNorm + ReLU (network.py:101-110): x from azsp_split_features (board_size x
 *   board_size), w_split [2 planes][9 taps][C out][32 in] f16 (input channels >= the network's zero), y in the tower's split layout
 *   with planes S = board_size + 2 (pad - 1): pad = 1 for Go, pad = 3 for Gomoku (network.py:101-105).  On the device: tailored
 *   weight-stationary stems for (board 9, C 128 or 64, pad 1) and (board 13, C 64, pad 3); every other board with pad 1 or 3, planes
 *   3 <= S <= 64 and C = 64, 128 or 256 on the wave-per-tile stem k_stem_spg (csrc/az_conv_spg.h; one wave per 16 couts x 32 positions,
 *   the embedding margin of pad 3 as zero fragments), AZSP_EINVAL otherwise.  The three tailored shapes run k_stem_spg too -- with
 *   BIT-IDENTICAL results -- when the call is small by azsp_small_batch_waves (counted on the output planes) AND that limit has been
 *   raised above its default of 1024: at the default the tailored stems keep every call (see azsp_small_batch_waves).  The host twin
 *   (tests/hosttwin) restates the tailored shapes only and refuses the others.
 * azsp_head_split: both heads in fp32 in one pass over the tower output (network.py:118-156): the two 1x1 convolutions + BatchNorm +
 *   ReLU (head_w [3][C], head_b [3]: npol policy planes first), policy Linear + softmax over all A actions (pol_fc_wt = the Linear's
 *   weight TRANSPOSED, [npol*S*S][A], inputs in nn.Flatten order), value Linear + ReLU + Linear + tanh (val_fc1_wt transposed
 *   [(3-npol)*S*S][F], val_fc2_w [F], val_fc2_b); priors float [boards][A], values float [boards].  Any (S, C) with C % 8 == 0. */
int azsp_split_features(const float* planes_dev, void* dst_dev, int64_t boards, int32_t board_size, int32_t in_channels,
                        uint32_t* range_rec_dev, void* stream);
int azsp_stem_split(const void* x_split32_dev, const void* w_split_dev, const float* bias_dev, void* y_dev, int64_t boards, int32_t board_size,
                    int32_t channels, int32_t pad, int32_t relu, uint32_t* range_rec_dev, void* stream);
/* azsp_stem_split for inputs whose lo plane is all zero -- values that are exact in f16, i.e. the engine's AZSP_FEAT_F16_SPLIT features (0 / 1
 * observation planes): the lo plane is neither loaded nor multiplied (its product is exactly zero), the result is identical to azsp_stem_split's.
 * The same shapes as azsp_stem_split, on the same kernels (the host twin: the tailored shapes only). */
int azsp_stem_split_exact(const void* x_split32_dev, const void* w_split_dev, const float* bias_dev, void* y_dev, int64_t boards, int32_t board_size,
                          int32_t channels, int32_t pad, int32_t relu, uint32_t* range_rec_dev, void* stream);
int azsp_head_split(const void* x_dev, const float* head_w_dev, const float* head_b_dev, const float* pol_fc_wt_dev, const float* pol_fc_b_dev,
                    const float* val_fc1_wt_dev, const float* val_fc1_b_dev, const float* val_fc2_w_dev, float val_fc2_b, float* priors_dev,
                    float* values_dev, int64_t boards, int32_t board_size, int32_t channels, int32_t num_actions, int32_t fc_units, int32_t npol,
                    void* stream);

/* Range record of the split-precision evaluator (sticky): *events_host = how many kernel lanes have met a value with |v| > 65504 (or
 * a NaN among the fp32 inputs of azsp_split_layout / azsp_split_features, recorded as +inf) since the last reset -- each such value was
 * clamped; the reference would have carried it: core/pipeline.py:91-123 evaluates in fp32 -- and *max_abs_host = the largest such |v|
 * (0 if none).  Either pointer may be NULL; reset != 0 clears the record.  Synchronises `stream`.
 * azsp_split_range_read reads the record the caller passed to the kernels as range_rec_dev (NULL = the per-device default record);
 * azsp_split_range_status reads the default record.  alpha_zero_amd.core.network.InferenceNet owns one record per network;
 * SelfPlayActor polls it at every harvest and, on an event, rescales the network's activations by a power of two (exact) or falls
 * back to the library's fp32 convolutions -- see InferenceNet.calibrate_activation_scale. */
int azsp_split_range_read(const uint32_t* range_rec_dev, uint32_t* events_host, float* max_abs_host, int32_t reset, void* stream);
int azsp_split_range_status(uint32_t* events_host, float* max_abs_host, int32_t reset, void* stream);

/* Small batches (round 6).  The weight-stationary kernels behind azsp_conv3x3_split / azsp_resblock_split give every board to ONE
 * workgroup (built for tens of thousands of boards per launch: 10 - 33 us however few boards there are).  A call whose output is at most
 * `waves` tiles of 16 couts x 32 positions (one wave each; a 17x17 x 64 board is 40 of them) runs the wave-per-tile kernel k_conv3x3_spg
 * instead (csrc/az_conv_spg.h: a board is spread over the chip; BIT-IDENTICAL results, so an evaluation does not depend on the batch it
 * arrives in) -- the batch-1 forwards of a drop-in uct_search (alpha_zero/core/mcts_v2.py:301-450 evaluates one leaf at a time).
 * Sets the process-wide limit and returns the previous one; a negative argument only queries.  Default 1024 (one wave per SIMD of an
 * MI355X: the measured crossover, profiles/r06_spg_ab.txt), or the environment variable AZSP_SPG_MAX_WAVES; 0 = always the
 * weight-stationary kernels -- except the odd last board of a (9, 128) convolution or a (9, 64) block, which their two-board workgroups
 * cannot take: it runs k_conv3x3_spg whatever the limit.  Shapes without a weight-stationary kernel (plane sizes 3 .. 64, 64 / 128 / 256 filters) always run
 * k_conv3x3_spg (beyond `waves`: k_conv3x3_spgw, 48-position tiles whose activations a workgroup shares through LDS).
 * azsp_stem_split / azsp_stem_split_exact obey the same limit on their three tailored shapes, but only once it exceeds the default:
 * 0 = always the tailored stems, a huge value = the wave-per-tile stem k_stem_spg at any board count, the default = the tailored stems:
 * a conservative choice, NOT a measured one (tools/stem_ab.py is the A/B that would decide it; no run of it is recorded). */
int64_t azsp_small_batch_waves(int64_t waves);

/* Replay sampling on the device (core/replay.py:72-83 UniformReplay.sample + core/pipeline.py:636-643: the batch
 * tensors and apply_random_transformation): out_states[b] = T_op(ring_states[idx[b]]) cast to state_dtype (AZSP_FEAT_I8 / F32 /
 * BF16 / F16), out_pi[b] = T_op(ring_pi[idx[b]]), out_z[b] = ring_z[idx[b]].  The ring is what azsp_harvest fills:
 * states int8 [capacity][channels][N][N], pi float [capacity][A], z float [capacity]; idx int64 [batch] (device); op as in
 * azsp_dihedral, one per batch like the reference.  One pass over HBM, no host round trip. */
int azsp_replay_gather(const int8_t* ring_states_dev, const float* ring_pi_dev, const float* ring_z_dev, const int64_t* idx_dev, int32_t batch,
                       int32_t channels, int32_t board_size, int32_t num_actions, int32_t op, int32_t state_dtype, void* out_states_dev,
                       float* out_pi_dev, float* out_z_dev, void* stream);
/* azsp_replay_gather plus the auxiliary rings of azsp_harvest_aux in the SAME launch: out_own[b] = T_op(ring_own[idx[b]]) as float
 * [batch][N][N] -- the same op as the state planes: an ownership map that is not turned with its board is a wrong target -- and
 * out_score[b] = ring_score[idx[b]], out_root_q[b] = ring_root_q[idx[b]], gathered like z.  ring_own int8 [capacity][N][N], ring_score and
 * ring_root_q float [capacity].  Each of the three ring / output pairs may be NULL (AZSP_EINVAL for a ring without its output or the
 * reverse); with all three NULL this is azsp_replay_gather. */
int azsp_replay_gather_aux(const int8_t* ring_states_dev, const float* ring_pi_dev, const float* ring_z_dev, const int64_t* idx_dev, int32_t batch,
                           int32_t channels, int32_t board_size, int32_t num_actions, int32_t op, int32_t state_dtype, void* out_states_dev,
                           float* out_pi_dev, float* out_z_dev, const int8_t* ring_own_dev, const float* ring_score_dev,
                           const float* ring_root_q_dev, float* out_own_dev, float* out_score_dev, float* out_root_q_dev, void* stream);
/* Weighted append to the replay ring (policy surprise weighting; no counterpart in the reference: opt-in): source row i is written
 *   c_i = floor(w_i) + (u_i < w_i - floor(w_i))
 * times, w_i = weights_dev[i] widened to double and clamped to [0, 2^20] (a NaN or negative weight gives 0 copies), u_i = uniforms_dev[i],
 * one float64 uniform in [0, 1) per row.  The copies go to the ring rows (added + ofs[i] + j) % capacity, j < c_i, ofs = the exclusive
 * prefix of c: the rows the reference's per-transition loop would write for the source repeated c_i times (np.repeat), `added` = the rows
 * written before this call.  If the copies outnumber the ring only the last `capacity` land.  Two launches on `stream`: one workgroup
 * counts and scans into ofs_dev int32[rows + 1] (ofs_dev[rows] = the total, which the caller reads to advance `added`; prefixes saturate
 * at INT32_MAX), then one flat kernel over the source elements reads each once and writes its copies.  The auxiliary ring / source pairs
 * of azsp_harvest_aux may each be NULL (AZSP_EINVAL for a ring without its source or the reverse).  Layouts as azsp_replay_gather_aux. */
int azsp_replay_add_weighted(int8_t* ring_states_dev, float* ring_pi_dev, float* ring_z_dev, int64_t capacity, int64_t added,
                             const int8_t* src_states_dev, const float* src_pi_dev, const float* src_z_dev, int32_t rows, int32_t channels,
                             int32_t board_size, int32_t num_actions, const float* weights_dev, const double* uniforms_dev, int8_t* ring_own_dev,
                             float* ring_score_dev, float* ring_root_q_dev, const int8_t* src_own_dev, const float* src_score_dev,
                             const float* src_root_q_dev, int32_t* ofs_dev, void* stream);

/* Stem of the evaluator (core/network.py:98-108 conv_block: conv3x3 17 -> C + BatchNorm + ReLU) on the tiled layout: the
 * input is the feature tensor azsp_select writes with feature_dtype = AZSP_FEAT_BF16_TILED (2K+1 planes, 17 at num_stack K = 8,
 * zero-padded to 32 channels: [tile][4][3*S*S][8] bf16, azsp_tiled_bytes(rows, S, 32) bytes); w_packed is [9 taps][C out][32 in] bf16
 * (input channels 2K+1..31 zero), the output is the tower's tiled layout with planes of board_size + 2 (pad - 1): pad = 1 for Go, pad = 3
 * for Gomoku (core/network.py:101-105: 13x13 boards become 17x17 planes).  Same kernels as azsp_conv3x3_tiled with 4 input chunks;
 * on the device: (board 9, 128 filters, pad 1), (board 9, 64 filters, pad 1), (board 13, 64 filters, pad 3) and (board 19, 256 filters, pad 1). */
int azsp_stem_tiled(const void* features_tiled_dev, const void* w_packed_dev, const float* bias_dev, void* y_tiled_dev, int64_t boards,
                    int32_t board_size, int32_t channels, int32_t pad, int32_t relu, void* stream);
/* Both 1x1 head convolutions (core/network.py:131-156: conv1x1 + BatchNorm + ReLU of the policy and the value head) in one
 * pass over the tiled tower output: w [policy_planes + value_planes][C] fp32 (BatchNorm folded), bias fp32;
 * pol_out [boards][policy_planes][S*S], val_out [boards][value_planes][S*S] bf16 (plane-major = nn.Flatten order); rows are
 * pol_stride / val_stride elements apart (0 = dense; azsp_fc_heads wants multiples of 16 with zero padding). */
int azsp_head_tiled(const void* x_tiled_dev, const float* w_dev, const float* bias_dev, void* pol_out_dev, void* val_out_dev, int64_t boards,
                    int32_t board_size, int32_t channels, int32_t policy_planes, int32_t value_planes, int32_t pol_stride, int32_t val_stride,
                    void* stream);
/* Fully connected layers of both heads with softmax / tanh (core/network.py:136-156 Linear layers, core/pipeline.py:105 softmax):
 * priors[b] = softmax(Wp pol[b] + bp) over A actions (fp32), values[b] = tanh(W2 relu(W1 val[b] + b1) + b2).  pol / val: bf16 rows
 * of k1_steps * 16 / k2_steps * 16 elements (zero padded), wp [ceil32(A)][k1_steps * 16] and w1 [ceil32(F)][k2_steps * 16] bf16
 * zero padded, bp / b1 / w2 fp32 padded to ceil32.  MFMA GEMMs, one wave per 32 boards; A <= 192, F <= 128 on the device. */
int azsp_fc_heads(const void* pol_dev, const void* val_dev, const void* wp_dev, const float* bp_dev, int32_t k1_steps, const void* w1_dev,
                  const float* b1_dev, int32_t k2_steps, const float* w2_dev, float b2, float* priors_dev, float* values_dev, int64_t boards,
                  int32_t num_actions, int32_t fc_width, void* stream);

/* f16 variants of the bf16 evaluator entries above: identical layouts, arguments and kernels, with f16 activations / weights / head
 * planes (the f16 MFMA runs at the bf16 rate and carries three more significand bits; outputs are clamped to f16's finite range).
 * Features: feature_dtype = AZSP_FEAT_F16_TILED.  On the device: the 9x9 x 128 evaluator ((S, C) = (9, 128), pad 1, 82 actions,
 * 128 fully connected units); AZSP_EINVAL for other shapes. */
int azsp_conv3x3_tiled_f16(const void* x_dev, const void* w_packed_dev, const float* bias_dev, const void* residual_dev, void* y_dev,
                           int64_t boards, int32_t board_size, int32_t channels, int32_t relu, void* stream);
int azsp_stem_tiled_f16(const void* features_tiled_dev, const void* w_packed_dev, const float* bias_dev, void* y_tiled_dev, int64_t boards,
                        int32_t board_size, int32_t channels, int32_t pad, int32_t relu, void* stream);
int azsp_head_tiled_f16(const void* x_tiled_dev, const float* w_dev, const float* bias_dev, void* pol_out_dev, void* val_out_dev, int64_t boards,
                        int32_t board_size, int32_t channels, int32_t policy_planes, int32_t value_planes, int32_t pol_stride,
                        int32_t val_stride, void* stream);
int azsp_fc_heads_f16(const void* pol_dev, const void* val_dev, const void* wp_dev, const float* bp_dev, int32_t k1_steps, const void* w1_dev,
                      const float* b1_dev, int32_t k2_steps, const float* w2_dev, float b2, float* priors_dev, float* values_dev, int64_t boards,
                      int32_t num_actions, int32_t fc_width, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AZSP_H */
