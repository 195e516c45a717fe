// az_engine.h -- batched PUCT self-play: one 64-lane wave owns one game (tree + real position).
//
// Restates, for thousands of concurrent games resident in HBM, the reference search and actor:
//   alpha_zero/core/mcts_v2.py   best_child :142-185, expand :188-210, backup :213-232,
//                                add_dirichlet_noise :235-262, generate_search_policy :265-298,
//                                uct_search :301-450, virtual loss :453-482, parallel_uct_search :485-657
//   alpha_zero/core/pipeline.py  play_and_record_one_game :289-382 (samples, resignation, z back-fill)
//   alpha_zero/envs/base.py      observation :228-259
// Data layout (per game, all in HBM):
//   node record  = [Hdr | N f32[AP] | W f32[AP] | P f32[AP] | child i16[AP] | hint i16[AP]]   (REC bytes, 128-B aligned rows)
//                  hint[a] = the node the search last continued to BELOW child a (a prefetch hint only, see descend())
//                  Hdr carries the position reached by the node, so a descent is an index walk and
//                  a child position is computed once, when the child is created (the reference
//                  re-steps a deep-copied env from the root on every simulation: mcts_v2.py:382-402)
//   GameRec      = real position, 8-deep board history, root statistics, per-round leaf table
// Numerics: every floating-point expression keeps the operand precision and evaluation order of the
// NumPy original (float32 rows, float64 noisy root priors, Python-double root statistics on a fresh
// root), compiled with -ffp-contract=off, so visit counts match the reference exactly.
#pragma once
#include "az_rules.h"
#include "az_dihedral.h"
#include <math.h>

#define AZ_MAXP 32        // max leaves per game per round (num_parallel)
#ifndef AZ_PATH_CAP
#define AZ_PATH_CAP 64    // tree levels handled lane-parallel (one lane per edge); deeper paths walk the parent links
#endif
#define AZ_INJ_K 16       // injected sampling uniforms per move
// GameRec::sim_budget: the low bits hold the slot's simulations per move, AZ_SB_FAST marks a fast move of the playout cap
#define AZ_SB_SIMS_MASK 0xFFFF
#define AZ_SB_FAST 0x10000
// ... and bits 17-31 how many simulations the decided-game visit reduction takes off the move in progress (azsp_set_visit_reduction; 0 on a
// fast move and with the rule off)
#define AZ_SB_CUT_SHIFT 17
#define AZ_VR_RING 8      // root values a slot remembers for the visit reduction
// stg_meta: bit 0 = black to move, AZ_META_FAST = the sample's move was a fast search of the playout cap
#define AZ_META_BLACK 1
#define AZ_META_FAST 2
// AzCfg::leaf_sym (azsp_set_leaf_symmetry): 0..7 = that dihedral op for every row, or one of these two
#define AZ_SYM_OFF (-1)
#define AZ_SYM_RANDOM (-2)
// GameRec::root_noisy: 0 = the float32 priors, 1 = rootP holds the float64 priors with Dirichlet noise, AZ_ROOT_GUMBEL = a Gumbel root:
// rootP holds the base row b(a) = g(a) + log P(a), gum_n0 the child N at search begin, and the root's selection is gumbel_child()
#define AZ_ROOT_GUMBEL 2

enum { AZS_NEED_ROOT = 0, AZS_SEARCH = 1, AZS_MOVE_DONE = 2, AZS_IDLE = 3, AZS_WAIT_BUF = 4 };
enum { AZ_ERR_NODES = 1, AZ_ERR_SAMPLE = 4, AZ_ERR_STAGE = 8 };  // bit 2 (tree depth) retired: deep paths walk parent links
enum { AZ_FEAT_I8 = 0, AZ_FEAT_F32 = 1, AZ_FEAT_BF16 = 2, AZ_FEAT_F16 = 3, AZ_FEAT_BF16_TILED = 4, AZ_FEAT_F16_TILED = 5, AZ_FEAT_F16_SPLIT = 6 };
enum { AZB_FREE = 0, AZB_FILLING = 1, AZB_COMPLETE = 2 };
// statistics counters (u64 each)
enum { AZC_SIMS = 0, AZC_NODE_VISITS, AZC_BACKUP_EDGES, AZC_LEAVES, AZC_DUP_LEAVES, AZC_TERMINAL_HITS, AZC_MOVES,
       AZC_GAMES, AZC_ROOT_EVALS, AZC_NODES_CREATED, AZC_ROUNDS, AZC_STALLS, AZC_HINT_PREFETCH, AZC_HINT_HITS, AZC_REDUCED_MOVES,
       AZC_COUNT = 16 };

AZ_HD u64 az_bits_f64(double v) {
    u64 b;
    __builtin_memcpy(&b, &v, sizeof b);
    return b;
}

struct AzCfg {
    int game, n, G, P, sims, budget, parallel_mode, max_nodes;
    int root_noise, deterministic, reuse_tree, warm_up_steps;
    int has_resign, check_resign_after, force_resign_disabled;  // force: -1 draw per game, 0/1 fixed
    int inject, inj_moves, stop_after_move, max_plies, stop_at_game_end;
    int feat_dtype, tab_len, log_moves, log_cap, stage_cap, training_steps;
    int K;  // num_stack: history boards per observation (1..8), 2K + 1 planes
    float one_minus_eps_f32, disable_resign_ratio;
    double eps, alpha, resign_threshold;
    RuleCfg rc;
    u64 seed;
    int rank;
    // playout cap (azsp_set_playout_cap; actor mode only, 0 = off): a move is a full search with probability cap_full_prob, else a
    // fast one of cap_fast simulations without root noise
    int cap_fast;
    double cap_full_prob;
    // leaf symmetry (azsp_set_leaf_symmetry; AZ_SYM_OFF = off): every feature row is written under a board symmetry, its priors are mapped
    // back when its node is expanded.  sym_live: AzMem::leaf_sym may hold a nonzero op -- the host sets it with the first mode that is
    // not off and clears it after a select over all games with the mode off again; while it is 0 neither phase touches leaf_sym.
    int leaf_sym, sym_live;
    // forced playouts at the root + policy-target pruning (azsp_set_forced_playouts; forced_k = 0: off).  A root child with n_eff > 0
    // visits (in-flight descents included) and n_eff^2 < forced_k * P * T_eff is selected before the PUCT arg-max; at the end of the move
    // the forced visits the search did not want are taken out of the recorded policy target (prune_target), not out of the tree.
    // A fast move of the playout cap is neither forced nor pruned.
    int prune_target;
    double forced_k;
    // Gumbel root search (azsp_set_gumbel; gumbel_m = 0: off; include/azsp.h states the rule).  gumbel_m = the most actions considered,
    // sigma(a) = (gumbel_cv + max N) * gumbel_cs * (completedQ(a) + 1) / 2.  Never on together with forced playouts.
    int gumbel_m;
    double gumbel_cv, gumbel_cs;
    // auxiliary training targets (azsp_set_aux_targets; 0 = off): record_sample stages the root value of the move, finalize_game the
    // owner bitboards of the final position.  AzMem::stg_own / stg_rootq are null until the first enabling call; once they exist, a
    // move or a game end with the feature off stages zeros, so that a harvest never reads what an earlier game left there.
    int aux;
    // policy surprise weighting (azsp_set_policy_surprise; 0 = off): record_sample stages the KL divergence of the recorded policy target
    // from the root's raw prior.  AzMem::stg_surprise is null until the first enabling call; once it exists, a move recorded with the
    // feature off stages 0.  (The game weights are the harvest's: OpHarvest.)
    int surprise;
    // decided-game visit reduction (azsp_set_visit_reduction; vr_L = 0: off; include/azsp.h states the rule).  AzMem::vr / stg_base are null
    // until the first enabling call.  vr_epoch counts the calls that turned the rule on: a slot whose VrSlot carries another epoch starts over.
    int vr_L, vr_min, vr_epoch;
    double vr_t, vr_w;
};

// per-slot state of the visit reduction: the ring of Black's root values, newest first, how many have been pushed, the prop of the move in progress
struct VrSlot {
    double ring[AZ_VR_RING];
    double prop;
    int seen, epoch;
};

struct AzMem {
    unsigned char* nodes;    // [G][max_nodes][REC]
    unsigned char* games;    // [G] GameRec
    double* rootP;           // [G][AP]   float64 root priors (after Dirichlet noise)
    int16_t* free_stack;     // [G][max_nodes]
    int* leaf_path;          // [G][P][AZ_PATH_CAP]  (node << 16) | move per edge, root first
    const double* pbc_np;    // [tab_len] pb_c for a node whose visit count is an np.float32
    const double* pbc_py;    // [tab_len] pb_c for a fresh root whose visit count is a Python float
    const float* sqrt32;     // [tab_len] float32(sqrt(n))
    const double* inj_noise; // [G][inj_moves][A]
    const double* inj_unif;  // [G][inj_moves][AZ_INJ_K]
    u64* stg_planes;         // [G][2][stage_cap][16][W]
    float* stg_pi;           // [G][2][stage_cap][A]
    unsigned char* stg_meta; // [G][2][stage_cap]   AZ_META_*
    int16_t* stg_move;       // [G][2][stage_cap]   the move played from the sample's position (-1 = resigned)
    int* stg_hdr;            // [G][2][16]  see SH_*
    u64* stg_own;            // [G][2][2][W]        owner bitboards (black, white) of the game's final position; null until azsp_set_aux_targets
    float* stg_rootq;        // [G][2][stage_cap]   root value of the sample's search, mover's perspective; null until azsp_set_aux_targets
    float* stg_surprise;     // [G][2][stage_cap]   KL(policy target || root prior) of the sample's search; null until azsp_set_policy_surprise
    float* stg_base;         // [G][2][stage_cap]   base weight of the sample (visit reduction); null until azsp_set_visit_reduction
    VrSlot* vr;              // [G]                 visit reduction: ring, seen, prop; null until azsp_set_visit_reduction
    // move log (tests / shim): per game per logged move
    double* log_pi;          // [G][log_cap][A]
    float* log_childN;       // [G][log_cap][A]
    double* log_q;           // [G][log_cap][4]  root_q, child_q, root_N before search (unused), move
    double* target_pi;       // [G][A]  policy target of the slot's last finished search (forced playouts: pruned; Gumbel: pi'); null until one of them is first enabled
    float* gum_n0;           // [G][AP] Gumbel root search: the root's child N when the slot's search began; null until the mode is first enabled
    uint8_t* leaf_sym;       // [G][P]  the dihedral op the row's features were written under (0 = as they are): select writes, expand reads
    u32* sym_rows;           // [G]     feature rows this slot has written under a leaf symmetry since azsp_create: a counter word of its op stream
    u64* counters;           // [G][AZC_COUNT]  per-game rows (no atomics: 4096 waves hammering 12 shared words cost ~0.6 ms per launch)
    int* err;                // [1]
};

enum { SH_STATE = 0, SH_LEN, SH_WINNER, SH_AREA_B, SH_AREA_W, SH_PASSES, SH_RESIGNED, SH_RESIGN_DISABLED, SH_MARKED,
       SH_COULD_WON, SH_MARKED_PLAYER, SH_UID, SH_TRAINING_STEPS, SH_REWARD, SH_LAST_PLAYER,
       SH_THR_LO, SH_THR_HI, SH_TS_END, SH_COUNT = 20 };  // THR_*: the game's own resign threshold (double bits); TS_END: weights tag at its end

template <int W> struct GameRec {
    EnvState<W> env;     // the real position (== the root node's position)
    u64 hist[8][2][W];   // boards, newest first; hist[0] is the current board (base.py:261-266)
    double root_W;       // DummyNode slots of the root (mcts_v2.py:56-62)
    double out_root_q, out_child_q;
    int root_N;
    int root, n_free, status, root_fresh, root_noisy, ply, n_leaves, root_eval_pending;
    int uid, num_passes, marked_player, resign_disabled, cur_buf, out_move, noise_pending, noise_ready, games_done, warm_override;
    // per-game actor state, read when the game starts like the reference actor does before every game (pipeline.py:232-246):
    double resign_thr;   // var_resign_threshold.value at game start (<= -1: no resignation in this game)
    int train_steps;     // training_steps of the weights in use at game start (pipeline.py:237, :271)
    int sim_budget;      // AZ_SB_*: the slot's own simulations per move (azsp_set_budgets, 0 = the engine's) and the class of the move in progress
    int gum_rootN0;      // Gumbel root search: root_N when the slot's search began (n_sched = max(1, simulations - this))
    int gum_m;           // Gumbel root search: m when the slot's search began
    int gum_move;        // Gumbel root search: a* of the slot's last finished search, -1 = none (no Gumbel search yet, or a fast move)
    int16_t leaf_node[AZ_MAXP];
    uint8_t leaf_depth[AZ_MAXP];
};


// Philox4x32-10 counter-based generator (production randomness: one independent stream per
// (seed, rank, game slot, game uid, ply, purpose, lane); replaces the actor's global np.random state).
struct Philox {
    static AZ_HD void round(u32 (&c)[4], u32 k0, u32 k1) {
        const u64 p0 = (u64)0xD2511F53u * c[0], p1 = (u64)0xCD9E8D57u * c[2];
        const u32 n0 = (u32)(p1 >> 32) ^ c[1] ^ k0, n1 = (u32)p1, n2 = (u32)(p0 >> 32) ^ c[3] ^ k1, n3 = (u32)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    }
    static AZ_HD void gen(u64 key, u32 c0, u32 c1, u32 c2, u32 c3, u32 (&out)[4]) {
        u32 c[4] = {c0, c1, c2, c3};
        u32 k0 = (u32)key, k1 = (u32)(key >> 32);
        for (int i = 0; i < 10; ++i) {
            round(c, k0, k1);
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
        for (int i = 0; i < 4; ++i) out[i] = c[i];
    }
    static AZ_HD double u01(u32 hi, u32 lo) {  // 53-bit uniform in [0,1)
        return (double)((((u64)hi << 32) | lo) >> 11) * (1.0 / 9007199254740992.0);
    }
};

#define AZ_LDS_NODES 1024  // parent table of the re-root pass lives in LDS up to this pool size

#define AZ_FREE_PREFETCH 64
typedef u64 __attribute__((may_alias)) u64a;  // word copies of typed records (no strict-aliasing assumptions)

// One node record staged from HBM into LDS in one burst (header + N / W / P / child rows).
template <int AP, int HW> struct StagedRec {
    float rN[AP], rW[AP], rP[AP];
    int16_t rC[AP];
    int16_t rH[AP];  // prefetch hints (never read by the search arithmetic)
    u64a hdrw[HW];  // header (position, parent, move, expanded); may_alias words, read back as Hdr
};

template <int W, int AP, int HW> struct Scratch {
    u64 planes[16][W];          // observation planes being assembled / history shift buffer
    int path[AZ_PATH_CAP];      // (node << 16) | move per edge of the current descent (first AZ_PATH_CAP levels)
    int anc[8];                 // node id at level (depth & 7): the last 8 nodes of the descent, for the history planes
    union {  // phase-private scratch: the end-of-move work and the select phase never overlap within a wave's launch
        struct {
            double pi[AP];              // search policy of the move being finished
            double cdf[AP];             // its running sum (np.cumsum order)
            float tmpf[AP];             // float32 policy terms (Gomoku)
            int16_t parent[AZ_LDS_NODES];
        };
        struct {
            StagedRec<AP, HW> nxt;  // select: speculatively staged record of the node the descent will probably reach one level further down
            // select, forced playouts (all of it under `parent`: no LDS added, and in LDS because the select kernel has no register to
            // spare): leaves of the current batch below root move a; T_eff = the sum of the root's child N + the leaves accepted into the
            // batch so far, -1 = not on for this search; the forced child of the root for the descent that starts now, -1 = none
            float fv[AP];  // (float: the lane's address is the one of the N / W / P rows; a byte row cost the kernel two more VGPRs)
            int teff, fsel;
            // select, Gumbel root (root_noisy == AZ_ROOT_GUMBEL): fv[a] = v(a) - n0(a), so that n(a) = N(a) + fv[a]; teff = t = sum n(a);
            // fsel = the considered child for the descent that starts now; gm = m' = min(m, legal actions); gsched = n_sched
            int gm, gsched;
        };
    };
    StagedRec<AP, HW> root;     // the root's record: staged ONCE per round, kept current in LDS while the P descents update it
    StagedRec<AP, HW> cur;      // the record of the node the current descent is looking at (levels >= 1)
    double rP64[AP];            // float64 root priors (noisy root only)
    float wpath[AZ_PATH_CAP];   // W and N of the chosen child at every level of the current descent, captured at selection
    float npath[AZ_PATH_CAP];   //   time: virtual loss / terminal backup then need no read-modify-write round trip
    u64 ancst[8][2][W];         // stones of the last 8 nodes of the descent (history planes without re-reading headers)
    u64 hist[8][2][W];          // the real game's board history, staged once per round
    u64 leafst[2][W];           // the leaf's stones while its observation planes are assembled
    int16_t freetop[AZ_FREE_PREFETCH];
    int free_base;              // freetop[i] == free_stack[free_base + i]
};

template <class Wv, int N, int GAME> struct Engine {
    typedef Wv Wave;
    typedef Rules<Wv, N> R;
    typedef BBOps<N> O;
    typedef typename O::B B;
    static constexpr int GAME_ID = GAME;
    static constexpr int NP = N * N;
    static constexpr int A = NP + (GAME == AZ_GO ? 1 : 0);
    static constexpr int W = O::W;
    static constexpr int AP = (A + 31) / 32 * 32;
    static constexpr int EPL = (AP + 63) / 64;
    typedef EnvState<W> S;
    typedef GameRec<W> GR;
    struct Hdr {
        S st;
        int16_t parent, move;
        uint8_t expanded, pad_[3];
    };
    static constexpr int HDR = ((int)sizeof(Hdr) + 127) / 128 * 128;
    static constexpr int HW = ((int)sizeof(Hdr) + 7) / 8;
    typedef Scratch<W, AP, HW> SC;
    static constexpr int REC = (HDR + 3 * AP * 4 + 2 * AP * 2 + 127) / 128 * 128;
    static constexpr int GREC = ((int)sizeof(GR) + 127) / 128 * 128;

    const AzCfg& c;
    const AzMem& m;
    const int g;
    SC& sc;
    GR& gr;
    u64 cnt[AZC_COUNT];
    // Hot wave-uniform scalars of the GameRec, cached in registers for the duration of a select / backup phase: every `gr.x` is a
    // global-memory access (a load + wait + readfirstlane, i.e. an L2 round trip in the middle of a dependent chain).  The first
    // version read root_fresh / root_noisy / the pb_c table inside EVERY arg-max and n_free / root_W in every leaf; doing the arg-max
    // twice showed it cost 36 % of the select kernel (tools/sel_abl.sh).  hot_load() / hot_store() bracket the phase.
    int hs_root, hs_rootN, hs_nfree, hs_fresh, hs_noisy;
    double hs_rootW;
    int hs_tabN;        // the visit count the cached root table entries below belong to (-1: none)
    double hs_tabPbc;
    float hs_tabSq;

    AZ_HD void hot_load() {
        hs_root = Wv::uni(gr.root);
        hs_rootN = Wv::uni(gr.root_N);
        hs_nfree = Wv::uni(gr.n_free);
        hs_fresh = Wv::uni(gr.root_fresh);
        hs_noisy = Wv::uni(gr.root_noisy);
        hs_rootW = Wv::uni(gr.root_W);
        hs_tabN = -1;
    }
    AZ_HD void hot_store() {
        if (Wv::first()) {
            gr.root = hs_root;
            gr.root_N = hs_rootN;
            gr.n_free = hs_nfree;
            gr.root_W = hs_rootW;
        }
        Wv::sync();
    }
    // pb_c(n) and sqrt(n) of a node with n visits (host tables, azsp_set_tables): a global load each -- issued by the caller as early
    // as n is known so that it overlaps the staging of the node's record
    AZ_HD void table_entry(int n, bool fresh, double& pbc, float& sq) const {
        const int ti = n < c.tab_len ? n : c.tab_len - 1;
        pbc = Wv::uni(fresh ? m.pbc_py[ti] : m.pbc_np[ti]);
        sq = Wv::uni(m.sqrt32[ti]);
    }

    // The root visit count that ends this game's search (mcts_v2.py:378 / :568): its own simulations per move -- the slot's value, the
    // playout cap's on a fast move, else the engine's, clamped into [1, sims] because pool and tables are sized for `sims` -- plus P in
    // parallel mode, as azsp_create derives c.budget.
    AZ_HD int game_budget() const { return game_sims() + (c.parallel_mode ? c.P : 0); }
    AZ_HD int game_sims() const {  // the simulations per move themselves
        const int sb = Wv::uni(gr.sim_budget);
        int s = (sb & AZ_SB_FAST) ? c.cap_fast : (sb & AZ_SB_SIMS_MASK);
        if (s == 0) s = c.sims;
        s = s < 1 ? 1 : (s > c.sims ? c.sims : s);
        s -= (int)((u32)sb >> AZ_SB_CUT_SHIFT);  // visit reduction: what begin_move_class() took off this move (0 with the rule off)
        return s < 1 ? 1 : s;
    }
    // Visit reduction: the slot's state, started over if the rule has been turned on since the slot last used it.  (first lane only)
    AZ_HD VrSlot& vr_slot() {
        VrSlot& v = m.vr[g];
        if (v.epoch != c.vr_epoch) {
            v.epoch = c.vr_epoch;
            v.seen = 0;
            v.prop = 0.0;
        }
        return v;
    }
    // prop of the move that starts now: how far beyond vr_t one and the same side has led in all of the newest vr_L searches, as a share
    // of 1 - vr_t.  float64 in exactly this operation order (include/azsp.h).
    AZ_HD double vr_prop(const VrSlot& v) const {
        const int L = c.vr_L;
        if (v.seen < L) return 0.0;
        double lo = v.ring[0], hi = v.ring[0];
        for (int i = 1; i < L; ++i) {
            lo = v.ring[i] < lo ? v.ring[i] : lo;
            hi = v.ring[i] > hi ? v.ring[i] : hi;
        }
        const double d = lo > 0.0 ? lo : (hi < 0.0 ? -hi : 0.0);
        double prop = d > c.vr_t ? (d - c.vr_t) / (1.0 - c.vr_t) : 0.0;
        if (prop > 1.0) prop = 1.0;
        return prop;
    }
    // A finished search of the batched actor pushes Black's view of its root value.  (first lane only)
    AZ_HD void vr_push(double rq) {
        VrSlot& v = vr_slot();
        for (int i = AZ_VR_RING - 1; i > 0; --i) v.ring[i] = v.ring[i - 1];
        v.ring[0] = gr.env.to_play == 0 ? rq : -rq;
        v.seen += 1;
    }
    // Playout cap: the class of the move that starts now, from the game's own counter-based stream (a counter word of its own: the
    // Dirichlet stream uses `| action`, move sampling `| 0xFFF`, the leaf symmetry 0xFFD -- row_symmetry()).  Returns the move's
    // noise_pending.  (first lane only)
    AZ_HD int begin_move_class() {
        int sb = gr.sim_budget & AZ_SB_SIMS_MASK;
        int noise = c.gumbel_m > 0 ? AZ_ROOT_GUMBEL : c.root_noise;  // noise_pending names what is due (apply_noise): 1 = Dirichlet noise, 2 = the Gumbel base row
        if (c.cap_fast > 0 && !c.stop_after_move) {
            u32 r[4];
            Philox::gen(c.seed + (u64)c.rank, (u32)g, (u32)gr.uid, ((u32)gr.ply << 12) | 0xFFEu, 0x2000u, r);
            if (!(Philox::u01(r[0], r[1]) < c.cap_full_prob)) {
                sb |= AZ_SB_FAST;
                noise = 0;
            }
        }
        if (m.vr && !c.stop_after_move) {  // visit reduction: no randomness; a fast move keeps cap_fast and stages its prop all the same
            VrSlot& v = vr_slot();
            double prop = 0.0;
            if (c.vr_L > 0) {
                prop = vr_prop(v);
                if (!(sb & AZ_SB_FAST)) {
                    int full = sb & AZ_SB_SIMS_MASK;
                    if (full == 0) full = c.sims;
                    full = full < 1 ? 1 : (full > c.sims ? c.sims : full);  // (as game_sims() clamps it)
                    const int mm = c.vr_min < full ? c.vr_min : full;
                    const int cut = (int)(prop * (double)(full - mm));
                    if (cut > 0) {
                        sb |= (int)((u32)cut << AZ_SB_CUT_SHIFT);
                        cnt[AZC_REDUCED_MOVES]++;
                    }
                }
            }
            v.prop = prop;
        }
        gr.sim_budget = sb;
        return noise;
    }

    // Leaf symmetry: the op of the feature row this slot writes now into row `slot` of its P, remembered in leaf_sym for the expand phase.
    // AZ_SYM_RANDOM draws floor(8 u) from a stream of its own: key seed + rank, counters (slot, rows this slot has written under a
    // symmetry, 0xFFD, 0x3000) -- neither uid nor ply, which stand still in drop-in mode.  Wave-uniform.  (select phase, c.sym_live)
    AZ_HD int row_symmetry(int slot) {
        int op = c.leaf_sym;
        if (op != AZ_SYM_OFF) {
            const u32 rows = Wv::uni(m.sym_rows[g]);
            if (op == AZ_SYM_RANDOM) {
                u32 r[4];
                Philox::gen(c.seed + (u64)c.rank, (u32)g, rows, 0xFFDu, 0x3000u, r);
                op = Wv::uni((int)(r[0] >> 29));  // floor(8 u01(r[0], r[1])): the top three bits of the 53-bit uniform
            }
            if (Wv::first()) m.sym_rows[g] = rows + 1u;
        }
        if (op < 0 || op > 7) op = 0;  // AZ_SYM_OFF while rows of an earlier mode drain
        if (Wv::first()) m.leaf_sym[(size_t)g * c.P + slot] = (uint8_t)op;
        Wv::sync();
        return op;
    }
    // The observation planes assembled in LDS become D_op of themselves: bit q of a plane is its old bit src_op(q).  A ballot over 64
    // positions IS a word of the new plane (the idiom of OpSetStates::plane_word); a plane's words are all read before any is replaced.
    // The emitters then write the row as they always do -- in the tiled layouts into the row's own sub-tile --, so with the symmetry off
    // their code is the code it was.  (planes 2K.. are uniform, the colour plane included: no symmetry moves them)
    AZ_HD void permute_planes(int op) {
#pragma unroll 1  // (an opt-in path inside the hot select kernel: one group of W ballots in the code, not 2K of them)
        for (int pl = 0; pl < 2 * c.K; ++pl) {
            u64 nw[W];
#pragma unroll
            for (int k = 0; k < W; ++k)
                nw[k] = Wv::ballot([&](int lane) -> bool {
                    const int q = lane + 64 * k;
                    if (q >= NP) return false;
                    const int p = az_dihedral_src(op, N, q / N, q % N);
                    return ((sc.planes[pl][p >> 6] >> (p & 63)) & 1ull) != 0;
                });
            Wv::sync();
            if (Wv::first())
                for (int k = 0; k < W; ++k) sc.planes[pl][k] = nw[k];
            Wv::sync();
        }
    }
    // priors entry a of the true orientation <- where position a lies in D_op(observation): src_inv(op)(a)
    static AZ_HD int sym_image(int op, int p) { return az_dihedral_src(az_dihedral_inv(op), N, p / N, p % N); }

    AZ_HD Engine(const AzCfg& c_, const AzMem& m_, int g_, SC& sc_)
        : c(c_), m(m_), g(g_), sc(sc_), gr(*(GR*)(m_.games + (size_t)g_ * GREC)) {
        for (int i = 0; i < AZC_COUNT; ++i) cnt[i] = 0;
    }

    // ---- addressing -------------------------------------------------------------------------
    AZ_HD unsigned char* rec(int node) const { return m.nodes + ((size_t)g * c.max_nodes + node) * REC; }
    AZ_HD Hdr& hdr(int node) const { return *(Hdr*)rec(node); }
    AZ_HD float* rowN(int node) const { return (float*)(rec(node) + HDR); }
    AZ_HD float* rowW(int node) const { return (float*)(rec(node) + HDR + AP * 4); }
    AZ_HD float* rowP(int node) const { return (float*)(rec(node) + HDR + 2 * AP * 4); }
    AZ_HD int16_t* rowC(int node) const { return (int16_t*)(rec(node) + HDR + 3 * AP * 4); }
    AZ_HD int16_t* rowH(int node) const { return (int16_t*)(rec(node) + HDR + 3 * AP * 4 + AP * 2); }
    AZ_HD double* rootP() const { return m.rootP + (size_t)g * AP; }
    AZ_HD int* leaf_path(int slot) const { return m.leaf_path + ((size_t)g * c.P + slot) * AZ_PATH_CAP; }
    AZ_HD void fail(int code) const {
        if (Wv::first()) *m.err |= code;
    }

    AZ_HD bool action_legal(const S& s, int a) const {
        if (a < NP) {
            const int wi = a >> 6;
            u64 word = 0;
            for (int i = 0; i < W; ++i) word = (i == wi) ? s.legal[i] : word;
            return (word >> (a & 63)) & 1ull;
        }
        return GAME == AZ_GO && !(s.flags & AZF_TERMINAL);  // go_engine.py:441 pass is always legal
    }

    // ---- node pool --------------------------------------------------------------------------
    AZ_HD int alloc_node() {  // (select phase: between hot_load() and hot_store())
        if (hs_nfree <= 0) {
            fail(AZ_ERR_NODES);
            return 0;
        }
        const int pos = hs_nfree - 1, rel = pos - Wv::uni(sc.free_base);
        const int idx = Wv::uni((rel >= 0 && rel < AZ_FREE_PREFETCH) ? (int)sc.freetop[rel] : (int)m.free_stack[(size_t)g * c.max_nodes + pos]);
        hs_nfree -= 1;
        cnt[AZC_NODES_CREATED]++;
        return idx;
    }
    AZ_HD void free_all_nodes() {
        int16_t* fs = m.free_stack + (size_t)g * c.max_nodes;
        const int mn = c.max_nodes;
        for (int base = 0; base < mn; base += AZ_WAVE)
            Wv::lanes([&](int lane) {
                const int i = base + lane;
                if (i < mn) {
                    fs[i] = (int16_t)(mn - 1 - i);  // pops yield 0,1,2,...
                    hdr(i).parent = -2;             // tag: not in use (see reroot)
                }
            });
        if (Wv::first()) {
            gr.n_free = mn;
            gr.root = -1;
        }
        Wv::sync();
    }

    // ---- game lifecycle ---------------------------------------------------------------------
    AZ_HD void stage_begin() {  // claim a staging buffer for the game that starts now
        int* sh = m.stg_hdr + ((size_t)g * 2 + gr.cur_buf) * SH_COUNT;
        if (Wv::first()) {
            sh[SH_STATE] = AZB_FILLING;
            sh[SH_LEN] = 0;
        }
    }
    AZ_HD void new_game() {
        if (Wv::first()) {
            R::reset(gr.env, GAME);
            if (GAME == AZ_GOMOKU) gr.env.flags = 0;
            gr.ply = 0;
            gr.num_passes = 0;
            gr.marked_player = -1;
            gr.uid = gr.games_done * c.G + g;
            gr.n_leaves = 0;
            gr.root_eval_pending = 0;
            gr.noise_pending = 0;
            gr.resign_thr = c.has_resign ? c.resign_threshold : -1.0;  // pipeline.py:241-242: re-read before every game
            gr.train_steps = c.training_steps;
            int rd = 1;  // pipeline.py:244-246
            if (c.force_resign_disabled >= 0) rd = c.force_resign_disabled;
            else if (c.has_resign && gr.resign_thr > -1.0) {
                u32 r[4];
                Philox::gen(c.seed + (u64)c.rank, (u32)g, (u32)gr.uid, 0u, 0x5E51u, r);
                rd = Philox::u01(r[0], r[1]) > (double)c.disable_resign_ratio ? 0 : 1;
            }
            gr.resign_disabled = rd;
            gr.status = AZS_NEED_ROOT;
            if (m.vr) vr_slot().seen = 0;
        }
        Wv::lanes([&](int lane) {
            u64* flat = &gr.hist[0][0][0];
            for (int t = lane; t < 16 * W; t += AZ_WAVE) flat[t] = 0;
        });
        Wv::sync();
        free_all_nodes();
        stage_begin();
        Wv::sync();
    }

    // ---- row arithmetic (operand precision of the NumPy original) ----------------------------
    // root W: Python float while the root is fresh, np.float32 after a re-root (mcts_v2.py:439-443)
    AZ_HD void root_add_W(double v) {  // (between hot_load() and hot_store())
        if (hs_fresh) hs_rootW = hs_rootW + v;
        else hs_rootW = (double)((float)hs_rootW + (float)v);
    }
    // Apply `delta` to W (and +1 to N when count) on every edge of a path and on the root slot.
    // Edge d (0 = root's child) receives delta * (-1)^(depth-1-d); the root receives delta*(-1)^depth.
    // One lane per edge: edges of one path are distinct (parent,move) slots, and the same slot is
    // always handled by the same lane (its depth), so program order == reference order per slot.
    AZ_HD void path_update(const int* path, int depth, int leaf, float delta, bool flip, bool count) {
        if (depth <= AZ_PATH_CAP) {
            Wv::lanes([&](int lane) {
                if (lane < depth) {
                    const int e = path[lane];
                    const int node = e >> 16, mv = e & 0xffff;
                    const float v = (flip && ((depth - 1 - lane) & 1)) ? -delta : delta;
                    float* w = rowW(node) + mv;
                    *w = *w + v;  // float32 += (mcts_v2.py:230 / :466 / :481)
                    if (count) {
                        float* n = rowN(node) + mv;
                        *n = *n + 1.0f;
                    }
                }
            });
            root_add_W((double)((flip && (depth & 1)) ? -delta : delta));
        } else {
            // deeper than the lane-parallel path store (rare): walk the parent links from the leaf, exactly like the
            // reference's `while isinstance(node, Node)` loop
            float v = delta;
            int node = leaf;
            for (int hops = 0; hops < c.max_nodes; ++hops) {
                const int parent = Wv::uni((int)hdr(node).parent), mv = Wv::uni((int)hdr(node).move);
                if (parent < 0) break;
                if (Wv::first()) {
                    float* w = rowW(parent) + mv;
                    *w = *w + v;
                    if (count) {
                        float* n = rowN(parent) + mv;
                        *n = *n + 1.0f;
                    }
                }
                if (flip) v = -v;
                node = parent;
            }
            root_add_W((double)v);
        }
        if (count) hs_rootN += 1;
        if (count) cnt[AZC_BACKUP_EDGES] += (u64)depth + 1;
        Wv::sync();
    }

    // ---- PUCT selection (mcts_v2.py:99-109, :142-185) -----------------------------------------
    // Stage one whole node record (header + N/W/P/child rows, + the float64 root priors) into LDS: all loads of the
    // burst are in flight together, so a tree level costs ONE HBM/L2 round trip instead of one per dependent field.
    typedef StagedRec<AP, HW> SR;
    AZ_HD void stage_node(int node, SR& dst, bool with_root_p) {
        const float* rn = rowN(node);
        const float* rw = rowW(node);
        const float* rp = rowP(node);
        const int16_t* rc = rowC(node);
        const int16_t* rh = rowH(node);
        const u64a* hw = (const u64a*)rec(node);
        const double* rp64 = rootP();
        Wv::lanes([&](int lane) {
            if (lane < HW) dst.hdrw[lane] = hw[lane];
            for (int a = lane; a < AP; a += AZ_WAVE) {
                dst.rN[a] = rn[a];
                dst.rW[a] = rw[a];
                dst.rP[a] = rp[a];
                dst.rC[a] = rc[a];
                dst.rH[a] = rh[a];
                if (with_root_p) sc.rP64[a] = rp64[a];
            }
        });
        Wv::sync();
    }
    // Two records in ONE burst: the node the descent moves to and the node it will probably reach next (its hint).  All loads of
    // both records are issued before the first LDS store, so the pair costs one HBM / L2 round trip.
    AZ_HD void stage_two(int na, SR& da, int nb, SR& db) {
        const unsigned char* ra = rec(na);
        const unsigned char* rb = rec(nb);
        Wv::lanes([&](int lane) {
            u64a ha = 0, hb = 0;
            if (lane < HW) {
                ha = ((const u64a*)ra)[lane];
                hb = ((const u64a*)rb)[lane];
            }
            float an[EPL], aw[EPL], ap[EPL], bn[EPL], bw[EPL], bp[EPL];
            int16_t ac[EPL], ah[EPL], bc[EPL], bh[EPL];
#pragma unroll
            for (int j = 0; j < EPL; ++j) {
                const int a = lane + AZ_WAVE * j;
                if (a < AP) {
                    an[j] = ((const float*)(ra + HDR))[a];
                    aw[j] = ((const float*)(ra + HDR + AP * 4))[a];
                    ap[j] = ((const float*)(ra + HDR + 2 * AP * 4))[a];
                    ac[j] = ((const int16_t*)(ra + HDR + 3 * AP * 4))[a];
                    ah[j] = ((const int16_t*)(ra + HDR + 3 * AP * 4 + AP * 2))[a];
                    bn[j] = ((const float*)(rb + HDR))[a];
                    bw[j] = ((const float*)(rb + HDR + AP * 4))[a];
                    bp[j] = ((const float*)(rb + HDR + 2 * AP * 4))[a];
                    bc[j] = ((const int16_t*)(rb + HDR + 3 * AP * 4))[a];
                    bh[j] = ((const int16_t*)(rb + HDR + 3 * AP * 4 + AP * 2))[a];
                }
            }
            if (lane < HW) {
                da.hdrw[lane] = ha;
                db.hdrw[lane] = hb;
            }
#pragma unroll
            for (int j = 0; j < EPL; ++j) {
                const int a = lane + AZ_WAVE * j;
                if (a < AP) {
                    da.rN[a] = an[j], da.rW[a] = aw[j], da.rP[a] = ap[j], da.rC[a] = ac[j], da.rH[a] = ah[j];
                    db.rN[a] = bn[j], db.rW[a] = bw[j], db.rP[a] = bp[j], db.rC[a] = bc[j], db.rH[a] = bh[j];
                }
            }
        });
        Wv::sync();
    }
    static AZ_HD const Hdr& hdr_of(const SR& r) { return *(const Hdr*)r.hdrw; }

    AZ_HD int puct_argmax(const SR& r, bool at_root, double pbc64, float sq32) {
        const S& s = hdr_of(r).st;
        const float pbc32 = (float)pbc64;
        const bool noisy = at_root && hs_noisy;
        u64 lg[W];
        for (int i = 0; i < W; ++i) lg[i] = Wv::uni(s.legal[i]);
        const bool pass_ok = GAME == AZ_GO && !(Wv::uni((int)s.flags) & AZF_TERMINAL);
        cnt[AZC_NODE_VISITS]++;
        return Wv::argmax_first([&](int lane, double& best, int& bi) {
            for (int j = 0; j < EPL; ++j) {
                const int a = lane + 64 * j;  // word index of point a is j, its bit is the lane
                if (a >= A) continue;
                if (!(a < NP ? (j < W && ((lg[j < W ? j : 0] >> lane) & 1ull) != 0) : pass_ok)) continue;
                const float n = r.rN[a], w = r.rW[a];
                const float q = w / (n > 0.0f ? n : 1.0f);
                const float rr = sq32 / (1.0f + n);
                double sco;
                if (noisy) {
                    const double u = (pbc64 * sc.rP64[a]) * (double)rr;  // float64 priors at the noisy root
                    sco = (double)(-q) + u;
                } else {
                    const float u = (pbc32 * r.rP[a]) * rr;
                    sco = (double)(-q + u);
                }
                if (bi < 0 || sco > best) {
                    best = sco;
                    bi = a;
                }
            }
        });
    }

    // First-play urgency reduction (azsp_set_fpu; include/azsp.h states the rule): puct_argmax with the value of an unvisited child
    // replaced.  qself = Q_self of the node r (descend<true> hands it down), red = r_root at the root of the search, r_tree below it.
    // on (wave-uniform): an unvisited child (N = 0) takes fpu - W in place of -q, with fpu = qself - red * sqrt(mass) and mass = the
    // float64 sum of the priors of the visited children -- the prior the u term uses --, a lane's own elements in ascending lane + 64 j,
    // then the butterfly of Wave::sum_f64.  At a noisy root the float64 fpu enters the float64 sum, everywhere else it is rounded to
    // float32 once.  !on: every expression is puct_argmax's.  Only select<GUM, true> (OpSelectFpu, OpSelectGumbelFpu) reaches this function: the one more
    // wave reduction and the three wave-uniform values do not fit the 128 VGPRs of the plain 9x9 select kernel (forced_child).
    AZ_HD int puct_argmax_fpu(const SR& r, bool at_root, double pbc64, float sq32, bool on, double red, double qself) {
        const S& s = hdr_of(r).st;
        const float pbc32 = (float)pbc64;
        const bool noisy = at_root && hs_noisy;
        u64 lg[W];
        for (int i = 0; i < W; ++i) lg[i] = Wv::uni(s.legal[i]);
        const bool pass_ok = GAME == AZ_GO && !(Wv::uni((int)s.flags) & AZF_TERMINAL);
        cnt[AZC_NODE_VISITS]++;
        double fpu64 = 0.0;
        if (on) {
            const double mass = Wv::sum_f64([&](int lane) -> double {
                double part = 0.0;
                for (int j = 0; j < EPL; ++j) {
                    const int a = lane + 64 * j;
                    if (a < A && r.rN[a] > 0.0f) part = part + (noisy ? sc.rP64[a] : (double)r.rP[a]);
                }
                return part;
            });
            fpu64 = qself - red * sqrt(mass);
        }
        const float fpu32 = (float)fpu64;
        return Wv::argmax_first([&](int lane, double& best, int& bi) {
            for (int j = 0; j < EPL; ++j) {
                const int a = lane + 64 * j;
                if (a >= A) continue;
                if (!(a < NP ? (j < W && ((lg[j < W ? j : 0] >> lane) & 1ull) != 0) : pass_ok)) continue;
                const float n = r.rN[a], w = r.rW[a];
                const float q = w / (n > 0.0f ? n : 1.0f);
                const float rr = sq32 / (1.0f + n);
                const bool plain = n > 0.0f || !on;
                double sco;
                if (noisy) {
                    const double u = (pbc64 * sc.rP64[a]) * (double)rr;
                    sco = (plain ? (double)(-q) : fpu64 - (double)w) + u;
                } else {
                    const float u = (pbc32 * r.rP[a]) * rr;
                    sco = (double)((plain ? -q : fpu32 - w) + u);
                }
                if (bi < 0 || sco > best) {
                    best = sco;
                    bi = a;
                }
            }
        });
    }

    // Forced playouts (KataGo, Wu 2019, 3.2) at the root: with n_eff(a) = N(a) + v(a) -- v(a) = leaves of the current batch whose path starts
    // with a (sc.fv): virtual loss touches W only, so the in-flight descents are counted here -- and T_eff = sum N + leaves of the batch,
    // a legal child is forced when n_eff > 0 and n_eff^2 < (k P(a)) T_eff, in float64 as written (no square root).  P(a) is the prior the
    // PUCT term uses: rootP at a noisy root, else the float32 prior.  Returns the forced child with the lowest index, -1 = none.
    // Runs in select() in front of every descent and leaves its result in sc.fsel; descend() reads that word after the root's arg-max.
    // The 9x9 select kernel sits at 126 of the 128 VGPRs of four waves per SIMD with every SGPR in use: one more wave-uniform value
    // that lives across the descent (the first versions kept T_eff and the forced child in registers, or branched inside puct_argmax)
    // tips the scheduler over that line and the kernel comes out at 142 to 186 VGPRs.
    AZ_HD int forced_child(const SR& r) {
        const S& s = hdr_of(r).st;
        u64 lg[W];
        for (int i = 0; i < W; ++i) lg[i] = Wv::uni(s.legal[i]);
        const bool pass_ok = GAME == AZ_GO && !(Wv::uni((int)s.flags) & AZF_TERMINAL);
        const double kk = c.forced_k, teff = (double)Wv::uni(sc.teff);
        const bool noisy = hs_noisy != 0;
        for (int j = 0; j < EPL; ++j) {
            const u64 fm = Wv::ballot([&](int lane) -> bool {
                const int a = lane + 64 * j;
                if (a >= A) return false;
                if (!(a < NP ? (j < W && ((lg[j < W ? j : 0] >> lane) & 1ull) != 0) : pass_ok)) return false;
                const double ne = (double)r.rN[a] + (double)sc.fv[a];
                if (!(ne > 0.0)) return false;
                const double p = noisy ? sc.rP64[a] : (double)r.rP[a];
                return ne * ne < (kk * p) * teff;
            });
            if (fm) return 64 * j + __builtin_ctzll(fm);
        }
        return -1;
    }

    // ---- Gumbel root search (Danihelka et al., ICLR 2022; include/azsp.h azsp_set_gumbel states the rule) ----------------------
    // The considered-visit sequence cv(t; m', n_sched): sequential halving over m' actions written as "the visit count the next
    // considered action must have after t root visits of this search".  Wave-uniform integer loop, no table.
    // Bounded whatever it is handed: m' <= A, n_sched and t within what a 16-bit simulation count allows, and once k has reached 2 -- e
    // and k no longer change -- the rest of the loop in closed form, so it runs at most L + 1 times.
    static AZ_HD int considered_visits(int t, int mp, int n_sched) {
        mp = mp > A ? A : mp;
        n_sched = n_sched < 1 ? 1 : (n_sched > AZ_SB_SIMS_MASK ? AZ_SB_SIMS_MASK : n_sched);
        t = t < 0 ? 0 : (t > 2 * AZ_SB_SIMS_MASK ? 2 * AZ_SB_SIMS_MASK : t);
        if (mp <= 1) return t;
        int L = 0;
        while ((1 << L) < mp) ++L;
        int k = mp, base = 0;
        for (;;) {
            int e = n_sched / (L * k);
            e = e < 1 ? 1 : e;
            if (t < e * k) return base + t / k;
            if (k == 2) return base + e * (t / (2 * e)) + (t % (2 * e)) / 2;
            t -= e * k;
            base += e;
            k = k / 2 < 2 ? 2 : k / 2;
        }
    }
    // completed Q and sigma of a root whose rows are rn / rw / rp (the staged record in select, the node's rows at the end of a move),
    // with the root's own W and N: sig = (c_visit + max_legal N) * c_scale, vmix = the value an unvisited child is completed with.
    // sigma(a) = sig * ((cq(a) + 1) / 2) with cq(a) = -W(a) / N(a) for a visited child, else vmix: gumbel_sigma().
    AZ_HD void gumbel_stats(const S& s, const float* rn, const float* rw, const float* rp, double root_w, int root_n, double& sig, double& vmix) {
        const int top = Wv::argmax_first([&](int lane, double& best, int& bi) {
            for (int a = lane; a < A; a += AZ_WAVE)
                if (action_legal(s, a) && (bi < 0 || (double)rn[a] > best)) {
                    best = (double)rn[a];
                    bi = a;
                }
        });
        const double max_n = (top >= 0 && top < A) ? (double)rn[top] : 0.0;
        const double T = Wv::sum_f64([&](int lane) -> double {
            double part = 0.0;
            for (int a = lane; a < A; a += AZ_WAVE) part += action_legal(s, a) ? (double)rn[a] : 0.0;
            return part;
        });
        const double sp = Wv::sum_f64([&](int lane) -> double {
            double part = 0.0;
            for (int a = lane; a < A; a += AZ_WAVE) part += (action_legal(s, a) && rn[a] > 0.0f) ? (double)rp[a] : 0.0;
            return part;
        });
        const double spq = Wv::sum_f64([&](int lane) -> double {
            double part = 0.0;
            for (int a = lane; a < A; a += AZ_WAVE)
                part += (action_legal(s, a) && rn[a] > 0.0f) ? (double)rp[a] * (-((double)rw[a] / (double)rn[a])) : 0.0;
            return part;
        });
        const double v_root = root_n > 0 ? root_w / (double)root_n : 0.0;
        vmix = sp > 0.0 ? (v_root + T * (spq / sp)) / (1.0 + T) : v_root;
        sig = (c.gumbel_cv + max_n) * c.gumbel_cs;
    }
    static AZ_HD double gumbel_sigma(float n, float w, double sig, double vmix) {
        const double cq = n > 0.0f ? -((double)w / (double)n) : vmix;
        return sig * ((cq + 1.0) / 2.0);
    }
    // The root's choice for the descent that starts now (select(), where forced_child runs; its state is in LDS for the same reason):
    // among the legal actions with n(a) == cv(t) the largest b(a) + sigma(a), lowest index on ties; if no action has that count, among
    // those with the smallest n(a).  n(a) = N(a) + sc.fv[a], b = sc.rP64.
    AZ_HD int gumbel_child(const SR& r) {
        const S& s = hdr_of(r).st;
        double sig, vmix;
        gumbel_stats(s, r.rN, r.rW, r.rP, hs_rootW, hs_rootN, sig, vmix);
        float want = (float)considered_visits(Wv::uni(sc.teff), Wv::uni(sc.gm), Wv::uni(sc.gsched));
        u64 hit = 0;
        for (int j = 0; j < EPL; ++j)
            hit |= Wv::ballot([&](int lane) -> bool {
                const int a = lane + 64 * j;
                return a < A && action_legal(s, a) && r.rN[a] + sc.fv[a] == want;
            });
        if (!hit) {
            const int low = Wv::argmax_first([&](int lane, double& best, int& bi) {
                for (int a = lane; a < A; a += AZ_WAVE) {
                    const double neg = -(double)(r.rN[a] + sc.fv[a]);
                    if (action_legal(s, a) && (bi < 0 || neg > best)) {
                        best = neg;
                        bi = a;
                    }
                }
            });
            if (low < 0 || low >= A) return -1;
            want = Wv::uni(r.rN[low] + sc.fv[low]);
        }
        const int mv = Wv::argmax_first([&](int lane, double& best, int& bi) {
            for (int a = lane; a < A; a += AZ_WAVE) {
                if (!action_legal(s, a) || r.rN[a] + sc.fv[a] != want) continue;
                const double sco = sc.rP64[a] + gumbel_sigma(r.rN[a], r.rW[a], sig, vmix);
                if (bi < 0 || sco > best) {
                    best = sco;
                    bi = a;
                }
            }
        });
        return mv < A ? mv : -1;
    }

    // One descent from the root.  Returns 0 = leaf reached (unexpanded, non-terminal), 1 = terminal.
    // On return `leaf_state` holds the leaf's position (used for the observation planes).
    // FPU (select<GUM, true> only): every arg-max is puct_argmax_fpu, with Q_self of the node it is at -- Tree.Q of the oracle: the root's
    // W / N as Python floats while it is fresh and as np.float32 after a re-root, below the root the float32 W / N of the edge the
    // descent came by, 0 without a visit -- and r_root at depth 0, r_tree below.  A Gumbel root chooses by gumbel_child(): no rule there.
    template <bool FPU = false> AZ_HD int descend(int& node_out, int& depth_out, S& leaf_state, int fpu_on = 0, double fpu_tree = 0.0,
                                                  double fpu_root = 0.0) {
        const int root = hs_root;
        int node = root, depth = 0, n_self = hs_rootN;
        if (hs_tabN != hs_rootN) {  // the root's table entries change only when its visit count does (terminal backups)
            table_entry(hs_rootN, hs_fresh != 0, hs_tabPbc, hs_tabSq);
            hs_tabN = hs_rootN;
        }
        double pbc64 = hs_tabPbc;
        float sq32 = hs_tabSq;
        // Speculation (performance only, never changes what is selected): every edge remembers the node the search last continued
        // to below its child (`hint`).  Moving to a child, its record AND the record of its hinted successor are fetched in one
        // burst; if the next arg-max then picks that successor, its record is already in LDS and a tree level costs no memory
        // round trip.  A prefetched record is only used when its node index equals the authoritative child index, and nothing
        // writes a node record between the prefetch and its use (one wave owns the game), so a stale hint merely wastes a load.
        int cur_is_nxt = 0;   // which LDS record holds `node` at levels >= 1: 0 = sc.cur, 1 = sc.nxt
        int spec = -1;        // node whose record sits in the OTHER record (valid when >= 0)
        double qself = 0.0;
        if (FPU && hs_rootN > 0) qself = hs_fresh ? hs_rootW / (double)hs_rootN : (double)((float)hs_rootW / (float)hs_rootN);
        for (;;) {
            const SR& r = depth == 0 ? sc.root : (cur_is_nxt ? sc.nxt : sc.cur);  // the root record lives in LDS for the whole round
            int mv;
            if (FPU)
                mv = puct_argmax_fpu(r, depth == 0, pbc64, sq32, fpu_on && !(depth == 0 && hs_noisy == AZ_ROOT_GUMBEL), depth == 0 ? fpu_root : fpu_tree,
                                     qself);
            else
                mv = puct_argmax(r, depth == 0, pbc64, sq32);
            if (depth == 0) {  // forced playouts (select()): a forced child of the root goes first
                const int f = Wv::uni(sc.fsel);
                mv = f >= 0 ? f : mv;
            }
            int child = Wv::uni((int)r.rC[mv]);
            const int hint = Wv::uni((int)r.rH[mv]);
            n_self = Wv::uni((int)r.rN[mv]);
            table_entry(n_self, false, pbc64, sq32);  // the child's pb_c / sqrt: in flight while its record is staged
            if (FPU) {
                const float wsel = Wv::uni(r.rW[mv]), nsel = Wv::uni(r.rN[mv]);
                qself = nsel > 0.0f ? (double)(wsel / nsel) : 0.0;
            }
            if (Wv::first()) {
                if (depth < AZ_PATH_CAP) {
                    sc.path[depth] = (node << 16) | mv;
                    sc.wpath[depth] = r.rW[mv];
                    sc.npath[depth] = r.rN[mv];
                }
                sc.anc[depth & 7] = node;
                const S& hs = hdr_of(r).st;
                for (int q = 0; q < 2; ++q)
                    for (int w = 0; w < W; ++w) sc.ancst[depth & 7][q][w] = hs.stones[q][w];
            }
            depth++;
            if (child < 0) {  // lazy child creation (mcts_v2.py:182-183); its position is computed once, here
                child = alloc_node();
                S ns;
                R::template step<GAME>(hdr_of(r).st, mv, c.rc, ns);
                if (Wv::first()) {
                    Hdr& h = hdr(child);
                    h.st = ns;
                    h.parent = (int16_t)node;
                    h.move = (int16_t)mv;
                    h.expanded = 0;
                    rowC(node)[mv] = (int16_t)child;
                    if (node == root) sc.root.rC[mv] = (int16_t)child;
                }
                note_hint(depth - 1, child);
                leaf_state = ns;
                node_out = child;
                depth_out = depth;
                Wv::sync();
                return (ns.flags & AZF_TERMINAL) ? 1 : 0;
            }
            note_hint(depth - 1, child);
            node = child;
            if (depth >= 2 && spec == child) {
                cur_is_nxt ^= 1;  // predicted: the record is already staged in the other buffer
                spec = -1;
                cnt[AZC_HINT_HITS]++;
            } else {
                SR& dst = depth == 1 ? sc.cur : (cur_is_nxt ? sc.nxt : sc.cur);
                if (depth == 1) cur_is_nxt = 0;
                SR& oth = cur_is_nxt ? sc.cur : sc.nxt;
                if (hint >= 0 && hint != node && hint < c.max_nodes) {
                    stage_two(node, dst, hint, oth);
                    spec = hint;
                    cnt[AZC_HINT_PREFETCH]++;
                } else {
                    stage_node(node, dst, false);
                    spec = -1;
                }
            }
            const SR& cr = cur_is_nxt ? sc.nxt : sc.cur;
            const Hdr& h = hdr_of(cr);
            const int hflags = Wv::uni((int)h.st.flags), hexp = Wv::uni((int)h.expanded);
            if ((hflags & AZF_TERMINAL) || !hexp) {
                leaf_state = R::uni_state(h.st);
                node_out = node;
                depth_out = depth;
                Wv::sync();
                return (hflags & AZF_TERMINAL) ? 1 : 0;
            }
        }
    }
    // The descent just moved from the node of path level `lvl` to `succ`: remember it on the edge ABOVE that node (the hint of the
    // grandparent's edge), in memory and in the LDS copy of the root record.
    AZ_HD void note_hint(int lvl, int succ) {
        if (lvl < 1 || lvl > AZ_PATH_CAP) return;
        if (Wv::first()) {
            const int e = sc.path[lvl - 1];
            const int gp = e >> 16, gmv = e & 0xffff;
            rowH(gp)[gmv] = (int16_t)succ;
            if (gp == hs_root) sc.root.rH[gmv] = (int16_t)succ;
        }
    }

    // Select-phase path update (virtual loss / terminal backup) from the values captured during the descent: plain stores,
    // no read-modify-write round trip.  The captured W / N ARE the memory contents (only this wave touches its game, and
    // nothing else ran since the capture), so the float32 results are identical to the in-memory += of the reference.
    AZ_HD void path_apply(int depth, int leaf, float delta, bool flip, bool count) {
        if (depth > AZ_PATH_CAP) {  // rare deep path: parent-link walk in memory, then refresh the LDS copy of the root
            path_update(sc.path, depth, leaf, delta, flip, count);
            stage_node(hs_root, sc.root, false);
            return;
        }
        const int root = hs_root;
        Wv::lanes([&](int lane) {
            if (lane < depth) {
                const int e = sc.path[lane];
                const int node = e >> 16, mv = e & 0xffff;
                const float v = (flip && ((depth - 1 - lane) & 1)) ? -delta : delta;
                const float w = sc.wpath[lane] + v;  // float32 += (mcts_v2.py:230 / :466)
                rowW(node)[mv] = w;
                if (node == root) sc.root.rW[mv] = w;
                if (count) {
                    const float n = sc.npath[lane] + 1.0f;
                    rowN(node)[mv] = n;
                    if (node == root) sc.root.rN[mv] = n;
                }
            }
        });
        root_add_W((double)((flip && (depth & 1)) ? -delta : delta));
        if (count) hs_rootN += 1;
        if (count) cnt[AZC_BACKUP_EDGES] += (u64)depth + 1;
        Wv::sync();
    }

    // ---- observation planes (base.py:228-259) -------------------------------------------------
    // board k plies back from `leaf`: the leaf, its ancestors up to the root, then the real-game history
    AZ_HD void gather_planes(int leaf, int depth, int me, const S* leaf_state = nullptr) {
        if (leaf_state) {  // register-resident position -> LDS, so that the per-lane plane pick is an LDS index, not scratch
            if (Wv::first())
                for (int q = 0; q < 2; ++q)
                    for (int w = 0; w < W; ++w) sc.leafst[q][w] = leaf_state->stones[q][w];
            Wv::sync();
        }
        Wv::lanes([&](int lane) {
            for (int t = lane; t < 16 * W; t += AZ_WAVE) {
                const int w = t % W, pc = t / W, k = pc >> 1, col = (pc & 1) ? 1 - me : me;
                u64 v;
                if (depth < 0) v = gr.hist[k][col][w];  // the real position: the history ring itself
                else if (k == 0) v = leaf_state ? sc.leafst[col][w] : hdr(leaf).st.stones[col][w];
                else if (k <= depth) v = sc.ancst[(depth - k) & 7][col][w];
                else v = sc.hist[k - depth][col][w];
                sc.planes[pc][w] = v;
            }
        });
        Wv::sync();
    }
    // History depth K = c.K < 8 (num_stack): the observation is [X_t, Y_t, ..., X_t-K+1, Y_t-K+1, C] (base.py:228-259), 2K + 1 planes.
    // gather_planes always assembles the 16 planes of K = 8; this rewrites planes 2K.. in LDS -- plane 2K becomes the colour plane (all
    // ones when black is to move), the rest zero -- so that the emitters below read the K-deep observation from the same 16 plane rows.
    // Kept out of the emitters: at K = 8 nothing here runs and the emitters' code is the one of the 17-plane engine.
    AZ_HD void stack_planes(int me) {
        if (c.K == 8) return;
        const int KK = 2 * c.K;
        const u64 colour = me == 0 ? ~0ull : 0ull;
        Wv::lanes([&](int lane) {
            for (int t = KK * W + lane; t < 16 * W; t += AZ_WAVE) sc.planes[t / W][t % W] = t / W == KK ? colour : 0ull;
        });
        Wv::sync();
    }
    // plain [2K+1][N][N] planes (after stack_planes): plane 16 -- the colour at K = 8 -- is never reached at K < 8
    template <class T> AZ_HD void emit_planes(T* out, T one, int me) {
        const int total = (2 * c.K + 1) * NP;
        const bool black = me == 0;
        Wv::lanes([&](int lane) {
            for (int e = lane; e < total; e += AZ_WAVE) {
                const int pl = e / NP, p = e - pl * NP;
                bool v = pl < 16 ? ((sc.planes[pl][p >> 6] >> (p & 63)) & 1ull) : black;
                out[e] = v ? one : (T)0;
            }
        });
    }
    // The evaluator's tiled input layout (include/azsp.h azsp_stem_tiled): [tile = T rows][4 chunks][T NP positions][8] bf16 (or f16) with
    // T = max(1, 256 / NP) boards per tile (3 at 9x9), the 2K + 1 planes (K = num_stack) zero-padded to 32 channels.  At K = 8: chunks 0..1 =
    // the 16 stone planes, chunk 2 = colour plane + 7 zeros; chunk 3 and the padding are never written (the tensor is zero-initialised by
    // its owner).  At K < 8 the same stores write the planes stack_planes left in LDS (colour in channel 2K, zeros above it) and chunk 2
    // gets zeros, so channels 2K + 1..31 are zero.
    // AZ_FEAT_F16_SPLIT = the input of the fp32-class evaluator's stem (include/azsp.h azsp_stem_split): the split layout
    // [row][plane: hi, lo][4 chunks][NP positions][8] f16 -- the same chunk strips with ONE board per tile and a second (lo) plane that is
    // never written: observation planes are 0 / 1, exactly representable in f16, so their lo halves are zero (the owner zero-initialises).
    template <int TBF, int PLANES> AZ_HD void emit_tiled_t(void* feat, int slot, int me, u32 one) {
        const size_t r = (size_t)g * c.P + slot, tile = r / TBF;
        const int sub = (int)(r - tile * TBF);
        uint16_t* base = (uint16_t*)feat + tile * (size_t)(PLANES * 4 * TBF * NP * 8) + (size_t)sub * NP * 8;
        const u32 black = (me == 0 && c.K == 8) ? one : 0u;  // channel 16: the colour plane at K = 8 only
        // One lane per POSITION (81 positions: lanes 0-63, then 0-16): the 16 plane words of its 64-position group are
        // wave-uniform LDS reads (broadcast), a stone is one bit-field extract, two planes make one dword (bf16 1.0 = 0x3F80) with two
        // multiply-adds, a chunk is one 16-byte store.  (The first version walked (chunk, position) pairs with 8 per-lane 64-bit
        // shifts each: 54 % of the select kernel, tools/sel_abl.sh.)
        Wv::lanes([&](int lane) {
            for (int p = lane; p < NP; p += AZ_WAVE) {
                const int w = p >> 6, b = p & 63;
                const bool hi_half = b >= 32;
                const u32 sh = (u32)(b & 31);
#pragma unroll
                for (int cc = 0; cc < 2; ++cc) {
                    u32 d[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const u64 w0 = sc.planes[cc * 8 + 2 * k][w], w1 = sc.planes[cc * 8 + 2 * k + 1][w];
                        const u32 x0 = hi_half ? (u32)(w0 >> 32) : (u32)w0, x1 = hi_half ? (u32)(w1 >> 32) : (u32)w1;
                        d[k] = ((x0 >> sh) & 1u) * one + ((x1 >> sh) & 1u) * (one << 16);
                    }
                    u32* o = (u32*)(base + ((size_t)cc * TBF * NP + p) * 8);
                    o[0] = d[0];
                    o[1] = d[1];
                    o[2] = d[2];
                    o[3] = d[3];
                }
                u32* o = (u32*)(base + ((size_t)2 * TBF * NP + p) * 8);
                o[0] = black;
                o[1] = 0u;
                o[2] = 0u;
                o[3] = 0u;
            }
        });
    }
    AZ_HD void write_features(void* feat, int slot, int me) {
        stack_planes(me);
        if (c.sym_live) {  // leaf symmetry (wave-uniform branches): the row's op is drawn and remembered, the planes in LDS are permuted
            const int op = row_symmetry(slot);
            if (op) permute_planes(op);
        }
        if (c.feat_dtype == AZ_FEAT_BF16_TILED || c.feat_dtype == AZ_FEAT_F16_TILED) {
            constexpr int TBF = (256 / NP) > 0 ? 256 / NP : 1;
            emit_tiled_t<TBF, 1>(feat, slot, me, c.feat_dtype == AZ_FEAT_F16_TILED ? 0x3C00u : 0x3F80u);  // 1.0 in f16 / bf16
            return;
        }
        if (c.feat_dtype == AZ_FEAT_F16_SPLIT) {
            emit_tiled_t<1, 2>(feat, slot, me, 0x3C00u);
            return;
        }
        const size_t row = ((size_t)g * c.P + slot) * (size_t)((2 * c.K + 1) * NP);
        switch (c.feat_dtype) {
            case AZ_FEAT_I8: emit_planes<int8_t>((int8_t*)feat + row, (int8_t)1, me); break;
            case AZ_FEAT_F32: emit_planes<u32>((u32*)feat + row, 0x3F800000u, me); break;
            case AZ_FEAT_BF16: emit_planes<uint16_t>((uint16_t*)feat + row, (uint16_t)0x3F80u, me); break;
            default: emit_planes<uint16_t>((uint16_t*)feat + row, (uint16_t)0x3C00u, me); break;
        }
    }
    // Leaf symmetry, end of a select phase: the rows this select did NOT write (from `written` on) get op 0, so leaf_sym always describes
    // the last select and is all zero once the mode is off again.
    AZ_HD void sym_end(int written) {
        if (!c.sym_live) return;
        uint8_t* srow = m.leaf_sym + (size_t)g * c.P;
        Wv::lanes([&](int lane) {
            if (lane >= written && lane < c.P) srow[lane] = 0;
        });
    }

    // ---- select phase -------------------------------------------------------------------------
    // GUM: the Gumbel root rule is compiled in.  The batched actor's select kernel has no register to spare (forced_child), so the rule
    // lives in an instantiation of its own (OpSelectGumbel), launched once the mode has been enabled; select<false> is the kernel it was.
    // FPU: the first-play urgency reduction is compiled in (puct_argmax_fpu), for the same reason in instantiations of its own
    // (OpSelectFpu = select<false, true>, OpSelectGumbelFpu = select<true, true>; they carry the rule's three values, so that AzCfg and
    // with it every kernel's argument block stay as they were), launched once azsp_set_fpu has enabled the rule; with fpu_on = 0 they
    // select what select<GUM, false> selects.
    template <bool GUM, bool FPU = false> AZ_HD void select(void* feat, unsigned char* valid, int fpu_on = 0, double fpu_tree = 0.0, double fpu_root = 0.0) {
        unsigned char* vrow = valid + (size_t)g * c.P;
        if (Wv::first()) {
            sc.free_base = -(1 << 30);  // no staged free-stack window yet
            sc.teff = sc.fsel = -1;     // forced playouts: not on (yet)
        }
        Wv::sync();
        const int status = Wv::uni(gr.status);
        hot_load();
        if (status == AZS_NEED_ROOT) {
            // mcts_v2.py:364-368: the root position itself is evaluated first
            if (hs_root < 0) {
                const int r = alloc_node();
                if (Wv::first()) {
                    Hdr& h = hdr(r);
                    h.st = gr.env;
                    h.parent = -1;
                    h.move = -1;
                    h.expanded = 0;
                }
                hs_root = r;
                Wv::sync();
            }
            gather_planes(hs_root, -1, gr.env.to_play);  // the root IS the real position: hist[0..7]
            write_features(feat, 0, gr.env.to_play);
            Wv::lanes([&](int lane) {
                if (lane < c.P) vrow[lane] = lane == 0 ? 1 : 0;
            });
            if (Wv::first()) {
                gr.root_eval_pending = 1;
                gr.n_leaves = 0;
            }
            cnt[AZC_ROOT_EVALS]++;
            sym_end(1);
            hot_store();
            return;
        }
        int nleaf = 0;
        // `while root.N < budget` (mcts_v2.py:378 / :568): a kept sub-tree whose root already has its budget's visits owes no simulation;
        // the next end-of-move phase finishes its move
        const int budget = game_budget();
        if (status == AZS_SEARCH && !Wv::uni(gr.noise_pending) && hs_rootN < budget) {
            int attempts = 0;
            {  // the next pops of the free stack, staged once per round
                const int base = hs_nfree - AZ_FREE_PREFETCH;
                const int16_t* fs = m.free_stack + (size_t)g * c.max_nodes;
                Wv::lanes([&](int lane) {
                    const int i = base + lane;
                    if (i >= 0) sc.freetop[lane] = fs[i];
                });
                if (Wv::first()) sc.free_base = base;
                // the root record and the real game's history: staged once, then kept current in LDS
                const u64* gh = &gr.hist[0][0][0];
                u64* lh = &sc.hist[0][0][0];
                Wv::lanes([&](int lane) {
                    for (int t = lane; t < 16 * W; t += AZ_WAVE) lh[t] = gh[t];
                });
                Wv::sync();
                stage_node(hs_root, sc.root, hs_noisy != 0);
            }
            // A Gumbel root is tested first: a search that began under that rule keeps it, whatever has been switched since, and
            // gumbel_child() reads nothing but what this branch writes
            if (GUM && hs_noisy == AZ_ROOT_GUMBEL) {  // Gumbel root: t, v(a) - n0(a), m' and n_sched of this select phase
                const float* n0 = m.gum_n0 + (size_t)g * AP;
                const S& rs = hdr_of(sc.root).st;
                const int sum = Wv::sum_i32([&](int lane) -> int {
                    int part = 0;
                    for (int a = lane; a < AP; a += AZ_WAVE) {
                        const float was = n0[a];
                        part += (int)sc.root.rN[a] - (int)was;
                        sc.fv[a] = -was;
                    }
                    return part;
                });
                const int legal = Wv::sum_i32([&](int lane) -> int {
                    int part = 0;
                    for (int a = lane; a < A; a += AZ_WAVE) part += action_legal(rs, a) ? 1 : 0;
                    return part;
                });
                const int sched = game_sims() - Wv::uni(gr.gum_rootN0), gm = Wv::uni(gr.gum_m);
                if (Wv::first()) {
                    sc.teff = sum;
                    sc.gm = legal < gm || gm < 1 ? legal : gm;
                    sc.gsched = sched < 1 ? 1 : sched;
                }
                Wv::sync();
            } else if (c.forced_k > 0.0 && !(Wv::uni(gr.sim_budget) & AZ_SB_FAST)) {  // forced playouts: T_eff and v(a) of this select phase
                const int sum = Wv::sum_i32([&](int lane) -> int {
                    int part = 0;
                    for (int a = lane; a < AP; a += AZ_WAVE) {
                        part += (int)sc.root.rN[a];
                        sc.fv[a] = 0.0f;
                    }
                    return part;
                });
                if (Wv::first()) sc.teff = sum;
                Wv::sync();
            }
            // mcts_v2.py:572: up to P leaves in at most 2P attempts, one after another (each descent
            // sees the virtual losses of the previous ones); uct_search (:378-418) is the P == 1 case
            const int max_att = c.parallel_mode ? 2 * c.P : 1;
            while (nleaf < c.P && attempts < max_att) {
                attempts++;
                int node, depth;
                S leaf;
                if (Wv::uni(sc.teff) >= 0) {  // (wave-uniform) forced playouts, or a Gumbel root
                    const int f = (GUM && hs_noisy == AZ_ROOT_GUMBEL) ? gumbel_child(sc.root) : forced_child(sc.root);
                    if (Wv::first()) sc.fsel = f;
                    Wv::sync();
                }
                const int term = descend<FPU>(node, depth, leaf, fpu_on, fpu_tree, fpu_root);
                cnt[AZC_SIMS]++;
                if (term) {
                    // mcts_v2.py:407-411 / :604-608: back up -reward, node stays unexpanded
                    cnt[AZC_TERMINAL_HITS]++;
                    if (Wv::first() && sc.teff >= 0) sc.teff += 1;  // (forced playouts) the hit goes through the root: not in flight, counted in N
                    path_apply(depth, node, (float)(-(int)leaf.reward), true, true);
                    if (!c.parallel_mode && hs_rootN < budget) attempts = 0;  // uct_search keeps looping (:378)
                    if (!c.parallel_mode && hs_rootN >= budget) break;
                    continue;
                }
                if (c.parallel_mode) path_apply(depth, node, 1.0f, false, false);  // add_virtual_loss :453-467
                int* lp = leaf_path(nleaf);
                Wv::lanes([&](int lane) {
                    if (lane < depth && lane < AZ_PATH_CAP) lp[lane] = sc.path[lane];
                });
                if (Wv::first()) {
                    gr.leaf_node[nleaf] = (int16_t)node;
                    gr.leaf_depth[nleaf] = (uint8_t)(depth < 255 ? depth : 255);
                }
                if (Wv::first() && sc.teff >= 0) {  // (forced playouts) this leaf is in flight below its root move
                    sc.fv[sc.path[0] & 0xffff] += 1.0f;
                    sc.teff += 1;
                }
                Wv::sync();
                const int me = leaf.to_play;
                gather_planes(node, depth, me, &leaf);
                write_features(feat, nleaf, me);
                nleaf++;
                cnt[AZC_LEAVES]++;
            }
        }
        Wv::lanes([&](int lane) {
            if (lane < c.P) vrow[lane] = lane < nleaf ? 1 : 0;
        });
        if (Wv::first()) gr.n_leaves = nleaf;
        sym_end(nleaf);
        hot_store();
    }

    // ---- expand + backup phase (mcts_v2.py:188-232, :616-625) -----------------------------------
    // op (leaf symmetry, wave-uniform): the row was evaluated on D_op(observation), so the node stores D_inv(op)(prior) -- board entry a
    // is gathered from where position a lies in the transformed board, the pass column stays.
    // SYM: an instantiation of its own behind the scalar branch of expand_node, the plain one is the code it was.
    AZ_HD void expand_node(int node, const float* prior, int op = 0) {
        if (op) expand_node_t<true>(node, prior, op);
        else expand_node_t<false>(node, prior, 0);
    }
    template <bool SYM> AZ_HD void expand_node_t(int node, const float* prior, int op) {
        float* rn = rowN(node);
        float* rw = rowW(node);
        float* rp = rowP(node);
        int16_t* rc = rowC(node);
        int16_t* rh = rowH(node);
        Wv::lanes([&](int lane) {
            for (int a = lane; a < AP; a += AZ_WAVE) {
                rp[a] = a < A ? prior[(SYM && a < NP) ? sym_image(op, a) : a] : 0.0f;  // stored unmasked, not renormalised (:209)
                rn[a] = 0.0f;
                rw[a] = 0.0f;
                rc[a] = -1;
                rh[a] = -1;
            }
        });
        if (Wv::first()) hdr(node).expanded = 1;
        Wv::sync();
    }
    AZ_HD int row_op(int slot) const { return c.sym_live ? Wv::uni((int)m.leaf_sym[(size_t)g * c.P + slot]) : 0; }
    AZ_HD void apply_outputs(const float* priors, const float* values) {
        const size_t row0 = (size_t)g * c.P;
        if (Wv::uni(gr.root_eval_pending)) {
            expand_node(Wv::uni(gr.root), priors + row0 * A, row_op(0));
            if (Wv::first()) {
                gr.root_N = 1;  // backup(root, value) on DummyNode slots: 0.0 + 1, 0.0 + value
                gr.root_W = (double)values[row0];
                gr.root_fresh = 1;
                gr.root_noisy = 0;
                gr.root_eval_pending = 0;
                gr.status = AZS_SEARCH;
                gr.noise_pending = begin_move_class();
            }
            Wv::sync();
            return;
        }
        const int nl = Wv::uni(gr.n_leaves);
        if (nl == 0) return;
        hot_load();
        for (int s = 0; s < nl; ++s) {
            const int node = Wv::uni((int)gr.leaf_node[s]), depth = Wv::uni((int)gr.leaf_depth[s]);
            const int* lp = leaf_path(s);
            if (c.parallel_mode) path_update(lp, depth, node, -1.0f, false, false);  // revert_virtual_loss :470-482
            if (Wv::uni((int)hdr(node).expanded)) {  // picked twice in one round: evaluation wasted (:621-622)
                cnt[AZC_DUP_LEAVES]++;
                continue;
            }
            expand_node(node, priors + (row0 + s) * A, row_op(s));
            path_update(lp, depth, node, values[row0 + s], true, true);
        }
        if (Wv::first()) gr.n_leaves = 0;
        hot_store();
    }

    // ---- Dirichlet noise at the root (mcts_v2.py:235-262) ---------------------------------------
    AZ_HD double gamma_sample(double alpha, u64 key, u32 c0, u32 c1, u32 c2) {
        // Marsaglia-Tsang for alpha+1, boosted by U^(1/alpha) (alpha < 1)
        const double d = alpha + 1.0 - 1.0 / 3.0, cc = 1.0 / sqrt(9.0 * d);
        for (u32 it = 0;; ++it) {
            u32 r[4], q[4];
            Philox::gen(key, c0, c1, c2, 2u * it, r);
            Philox::gen(key, c0, c1, c2, 2u * it + 1u, q);
            const double u1 = Philox::u01(r[0], r[1]) + 1.0 / 18014398509481984.0, u2 = Philox::u01(r[2], r[3]);
            const double x = sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
            const double v0 = 1.0 + cc * x;
            if (v0 <= 0.0) continue;
            const double v = v0 * v0 * v0, u = Philox::u01(q[0], q[1]) + 1.0 / 18014398509481984.0;
            if (log(u) < 0.5 * x * x + d - d * v + d * log(v) || it > 64) {
                const double ub = Philox::u01(q[2], q[3]) + 1.0 / 18014398509481984.0;
                return d * v * exp(log(ub) / alpha);
            }
        }
    }
    // Gumbel(0, 1) draw of (game uid, ply, action) from the slot's counter-based stream: g = -log(-log u), u = (k + 1/2) 2^-52 with k
    // the top 52 bits of a Philox word pair, so 0 < u < 1 exactly.  Counter word 0x4000: the Dirichlet stream of the same (ply, action)
    // uses 0, 1, 2, ...
    AZ_HD double gumbel_draw(u64 key, u32 uid, int ply, int a) const {
        u32 r[4];
        Philox::gen(key, (u32)g, uid, ((u32)ply << 12) | (u32)a, 0x4000u, r);
        const double u = ((double)((((u64)r[0] << 32) | r[1]) >> 12) + 0.5) * (1.0 / 4503599627370496.0);
        return -log(-log(u));
    }
    // The start of a Gumbel root search, where apply_noise() adds the Dirichlet noise otherwise: the base row
    // b(a) = g(a) + log(max((double)P(a), 1e-45)) into the slot's float64 root row, and the snapshot n0 / root_N of the kept visits.
    // g(a) is the injected row (azsp_set_injection, azsp_begin_move[s]) or the slot's own draw.  The priors stay as they are.
    AZ_HD void apply_gumbel() {
        const int root = gr.root;
        const float* rp = rowP(root);
        const float* rn = rowN(root);
        double* rp64 = rootP();
        float* n0 = m.gum_n0 + (size_t)g * AP;
        const double* inj = c.inject ? m.inj_noise + ((size_t)g * c.inj_moves + (gr.ply < c.inj_moves ? gr.ply : c.inj_moves - 1)) * A : nullptr;
        const u64 key = c.seed + (u64)c.rank;
        const u32 uid = (u32)gr.uid;
        const int ply = gr.ply;
        Wv::lanes([&](int lane) {
            for (int a = lane; a < AP; a += AZ_WAVE) {
                double v = 0.0;
                if (a < A) {
                    const double p = (double)rp[a];
                    v = (inj ? inj[a] : gumbel_draw(key, uid, ply, a)) + log(p > 1e-45 ? p : 1e-45);
                }
                rp64[a] = v;
                n0[a] = rn[a];
            }
        });
        if (Wv::first()) {
            gr.root_noisy = AZ_ROOT_GUMBEL;
            gr.noise_pending = 0;
            gr.gum_rootN0 = gr.root_N;
            gr.gum_m = c.gumbel_m;  // (0 if the mode was switched off since the move was classed: every legal action is considered)
        }
        Wv::sync();
    }
    AZ_HD void apply_noise() {
        if (Wv::uni(gr.noise_pending) == AZ_ROOT_GUMBEL) {  // what the move was classed as when it began, not what the mode is now
            apply_gumbel();
            return;
        }
        const int root = gr.root;
        const S& s = hdr(root).st;
        const float* rp = rowP(root);
        double* rp64 = rootP();
        const double* inj = c.inject ? m.inj_noise + ((size_t)g * c.inj_moves + (gr.ply < c.inj_moves ? gr.ply : c.inj_moves - 1)) * A : nullptr;
        double total = 1.0;
        if (!c.inject) {
            // Dirichlet(alpha) over ALL actions = normalised Gamma(alpha) draws (:259-260)
            const u64 key = c.seed + (u64)c.rank;
            const double part = Wv::sum_f64([&](int lane) -> double {
                double acc = 0.0;
                for (int a = lane; a < A; a += AZ_WAVE) {
                    const double gsample = gamma_sample(c.alpha, key, (u32)g, (u32)gr.uid, ((u32)gr.ply << 12) | (u32)a);
                    rp64[a] = gsample;
                    acc += gsample;
                }
                return acc;
            });
            Wv::sync();
            total = part > 0.0 ? part : 1.0;
        }
        Wv::lanes([&](int lane) {
            for (int a = lane; a < AP; a += AZ_WAVE) {
                double v = 0.0;
                if (a < A) {
                    const double nz = c.inject ? inj[a] : rp64[a] / total;
                    // child_P * (1 - eps) stays float32, noise * eps is float64, the sum is float64 (:262)
                    v = (double)(rp[a] * c.one_minus_eps_f32) + (action_legal(s, a) ? nz : 0.0) * c.eps;
                }
                rp64[a] = v;
            }
        });
        if (Wv::first()) {
            gr.root_noisy = 1;
            gr.noise_pending = 0;
        }
        Wv::sync();
    }

    // Diagnostics (azsp_rng_probe): the production random streams of this slot for plies 0..plies-1 of its current game, drawn
    // exactly as apply_noise / sample_move draw them, without touching any state.
    AZ_HD void probe_rng(double* noise, double* unif, int plies, int tries) {
        const u64 key = c.seed + (u64)c.rank;
        const u32 uid = (u32)Wv::uni((int)gr.uid);
        for (int ply = 0; ply < plies; ++ply) {
            if (noise && c.gumbel_m > 0) {  // Gumbel root search on: the rows are the g(a) apply_gumbel draws
                double* row = noise + ((size_t)g * plies + ply) * A;
                Wv::lanes([&](int lane) {
                    for (int a = lane; a < A; a += AZ_WAVE) row[a] = gumbel_draw(key, uid, ply, a);
                });
            } else if (noise) {
                double* row = noise + ((size_t)g * plies + ply) * A;
                const double tot = Wv::sum_f64([&](int lane) -> double {
                    double acc = 0.0;
                    for (int a = lane; a < A; a += AZ_WAVE) {
                        const double gs = gamma_sample(c.alpha, key, (u32)g, uid, ((u32)ply << 12) | (u32)a);
                        row[a] = gs;
                        acc += gs;
                    }
                    return acc;
                });
                Wv::sync();
                Wv::lanes([&](int lane) {
                    for (int a = lane; a < A; a += AZ_WAVE) row[a] = row[a] / (tot > 0.0 ? tot : 1.0);
                });
            }
            if (unif) {
                Wv::lanes([&](int lane) {
                    for (int t = lane; t < tries; t += AZ_WAVE) {
                        u32 r[4];
                        Philox::gen(key, (u32)g, uid, ((u32)ply << 12) | 0xFFFu, 0x1000u + (u32)t, r);
                        unif[((size_t)g * plies + ply) * tries + t] = Philox::u01(r[0], r[1]);
                    }
                });
            }
        }
        Wv::sync();
    }

    // ---- end of a search: policy, move, sample, env step, re-root ---------------------------------
    static AZ_HD float pairwise_sum_f32(const float* a, int n) {
        // numpy's float32 add.reduce order (pairwise, 8 accumulators, blocks of 128), so that the
        // Gomoku policy (float32 in the reference) sums in the same order
        if (n < 8) {
            float r = 0.0f;
            for (int i = 0; i < n; ++i) r = r + a[i];
            return r;
        }
        if (n <= 128) {
            float r[8];
            for (int j = 0; j < 8; ++j) r[j] = a[j];
            int i = 8;
            for (; i < n - (n % 8); i += 8)
                for (int j = 0; j < 8; ++j) r[j] = r[j] + a[i + j];
            float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
            for (; i < n; ++i) res = res + a[i];
            return res;
        }
        int n2 = n / 2;
        n2 -= n2 % 8;
        return pairwise_sum_f32(a, n2) + pairwise_sum_f32(a + n2, n - n2);
    }

    // generate_search_policy (mcts_v2.py:265-298) into the wave's LDS row sc.pi[A] (and the move log when enabled).
    // rn: the visit counts the policy is formed from -- the root's child N, or the pruned counts of prune_counts() (an LDS row).
    AZ_HD void search_policy(bool warm, double* log_pi, const float* rn = nullptr) {
        const S& s = hdr(gr.root).st;
        if (!rn) rn = rowN(gr.root);
        if (GAME == AZ_GO) {
            // legal(int64) * child_N(float32) -> float64; n**5 and the sum are exact integers in float64, so the
            // summation order is irrelevant and a wave reduction is bit-identical to np.sum
            const double sum = Wv::sum_f64([&](int lane) -> double {
                double part = 0.0;
                for (int a = lane; a < A; a += AZ_WAVE) {
                    double x = action_legal(s, a) ? (double)rn[a] : 0.0;
                    if (!warm) {
                        const double x2 = x * x;
                        x = x2 * x2 * x;
                    }
                    sc.pi[a] = x;
                    part += x;
                }
                return part;
            });
            Wv::sync();
            if (sum > 0.0) {
                Wv::lanes([&](int lane) {
                    for (int a = lane; a < A; a += AZ_WAVE) sc.pi[a] = sc.pi[a] / sum;
                });
            }
        } else {
            // legal(int8) * child_N(float32) stays float32 (Gomoku); np.sum order = pairwise_sum_f32
            Wv::lanes([&](int lane) {
                for (int a = lane; a < A; a += AZ_WAVE) {
                    float x = action_legal(s, a) ? rn[a] : 0.0f;
                    if (!warm) {
                        const double d = (double)x, d2 = d * d;
                        x = (float)(d2 * d2 * d);
                    }
                    sc.tmpf[a] = x;
                }
            });
            Wv::sync();
            const float sum = pairwise_sum_f32(sc.tmpf, A);
            Wv::lanes([&](int lane) {
                for (int a = lane; a < A; a += AZ_WAVE) {
                    const float x = sc.tmpf[a];
                    sc.pi[a] = (double)(sum > 0.0f ? x / sum : x);
                }
            });
        }
        Wv::sync();
        if (log_pi) {
            Wv::lanes([&](int lane) {
                for (int a = lane; a < A; a += AZ_WAVE) log_pi[a] = sc.pi[a];
            });
        }
    }

    // Policy-target pruning (forced playouts; end of a search, no virtual loss outstanding) into the LDS row `out` (AP floats).
    // c* = the first legal action with the largest N, S* = its PUCT score; score(a, m) = the expression puct_argmax evaluates at the root
    // with N(a) replaced by m (q stays W(a) / N(a); pb_c, sqrt entry, float64 / float32 as at the root's final visit count).  Every other
    // visited legal child loses up to f(a) = floor(sqrt(k P(a) T)) visits, one at a time while its score stays below S*; a child left
    // with a single playout is pruned outright.  One lane per action, at most f(a) + 1 scores each.
    AZ_HD void prune_counts(float* out) {
        const int root = gr.root;
        const S& s = hdr(root).st;
        const float* rn = rowN(root);
        const float* rw = rowW(root);
        const float* rp = rowP(root);
        const double* rp64 = rootP();
        const bool noisy = Wv::uni(gr.root_noisy) != 0;
        double pbc64;
        float sq32;
        table_entry(Wv::uni(gr.root_N), Wv::uni(gr.root_fresh) != 0, pbc64, sq32);
        const float pbc32 = (float)pbc64;
        const double kk = c.forced_k;
        auto score = [&](int a, float n) -> double {
            const float n0 = rn[a], w = rw[a];
            const float q = w / (n0 > 0.0f ? n0 : 1.0f);
            const float rr = sq32 / (1.0f + n);
            if (noisy) return (double)(-q) + (pbc64 * rp64[a]) * (double)rr;
            return (double)(-q + (pbc32 * rp[a]) * rr);
        };
        const double T = Wv::sum_f64([&](int lane) -> double {
            double part = 0.0;
            for (int a = lane; a < A; a += AZ_WAVE) part += (double)rn[a];
            return part;
        });
        const int cs = Wv::argmax_first([&](int lane, double& best, int& bi) {
            for (int a = lane; a < A; a += AZ_WAVE)
                if (action_legal(s, a) && (bi < 0 || (double)rn[a] > best)) {
                    best = (double)rn[a];
                    bi = a;
                }
        });
        const bool any = cs >= 0 && cs < A && rn[cs] > 0.0f;
        const double sstar = any ? score(cs, rn[cs]) : 0.0;
        Wv::lanes([&](int lane) {
            for (int a = lane; a < AP; a += AZ_WAVE) {
                float keep = a < A ? rn[a] : 0.0f;
                if (any && a < A && a != cs && keep > 0.0f && action_legal(s, a)) {
                    const int ni = (int)keep;
                    // only min(f, N(a)) is used, and that is the largest integer with f^2 <= min(x, N(a)^2): the square root is taken of
                    // a value of at most N(a)^2 < 2^48 (N is a float32 count), whatever k is -- x itself may be huge or inf for a large k
                    const double nn = (double)ni * (double)ni, xk = (kk * (noisy ? rp64[a] : (double)rp[a])) * T;
                    const double x = xk < nn ? xk : nn;
                    int f = 0;  // a truncated square root, corrected with the multiplication; 0 <= f <= N(a)
                    if (x > 0.0) {
                        f = (int)sqrt(x);
                        while (f > 0 && (double)f * (double)f > x) --f;
                        while (f < ni && (double)(f + 1) * (double)(f + 1) <= x) ++f;
                    }
                    const int lo = ni - f;
                    int last = ni;
                    for (int mm = ni - 1; mm >= lo; --mm) {
                        if (score(a, (float)mm) >= sstar) break;
                        last = mm;
                    }
                    if (last < ni && last == 1) last = 0;
                    keep = (float)last;
                }
                out[a] = keep;
            }
        });
        Wv::sync();
    }
    // The policy target of the search that just ended (forced playouts on): the pruned policy unless the move was a fast one of the
    // playout cap or pruning is off -- then the plain one search_policy left in sc.pi.  It replaces sc.pi, which record_sample stages,
    // and goes to the slot's target_pi row.  (after the move was chosen from the unpruned policy; sc.cur is free at the end of a move)
    AZ_HD void make_target(bool warm) {
        if (c.prune_target && !(Wv::uni(gr.sim_budget) & AZ_SB_FAST)) {
            prune_counts(sc.cur.rN);
            search_policy(warm, nullptr, sc.cur.rN);
        }
        double* tp = m.target_pi + (size_t)g * A;
        Wv::lanes([&](int lane) {
            for (int a = lane; a < A; a += AZ_WAVE) tp[a] = sc.pi[a];
        });
        Wv::sync();
    }

    // End of a Gumbel root search (no virtual loss outstanding): a* = the largest b(a) + sigma(a) among the legal actions with the largest
    // N(a) - n0(a) -- and N(a) > 0 where the search made no simulation and a visited child exists --, lowest index on ties, into gr.gum_move; pi'(a) = softmax over the legal actions of log(max(P, 1e-45)) + sigma(a),
    // maximum subtracted first, float64, into sc.pi -- which record_sample stages -- and the slot's target_pi row.  The logs keep the
    // plain visit policy search_policy wrote.  Returns a*.  (sc.cdf is free: no move is sampled in this mode)
    AZ_HD int gumbel_target() {
        const int root = gr.root;
        const S& s = hdr(root).st;
        const float* rn = rowN(root);
        const float* rw = rowW(root);
        const float* rp = rowP(root);
        const double* b = rootP();
        const float* n0 = m.gum_n0 + (size_t)g * AP;
        double sig, vmix;
        gumbel_stats(s, rn, rw, rp, Wv::uni(gr.root_W), Wv::uni(gr.root_N), sig, vmix);
        const int most = Wv::argmax_first([&](int lane, double& best, int& bi) {
            for (int a = lane; a < A; a += AZ_WAVE)
                if (action_legal(s, a) && (bi < 0 || (double)(rn[a] - n0[a]) > best)) {
                    best = (double)(rn[a] - n0[a]);
                    bi = a;
                }
        });
        int astar = -1;
        if (most >= 0 && most < A) {
            const float want = Wv::uni(rn[most] - n0[most]);
            // a search that made no simulation (the kept sub-tree already held the budget): among the visited children, if there is
            // one, so that the move has a child node as a sampled move always has
            bool seen = false;
            if (want == 0.0f)
                for (int j = 0; j < EPL; ++j)
                    seen = seen || Wv::ballot([&](int lane) -> bool {
                               const int a = lane + 64 * j;
                               return a < A && action_legal(s, a) && rn[a] > 0.0f;
                           }) != 0;
            astar = Wv::argmax_first([&](int lane, double& best, int& bi) {
                for (int a = lane; a < A; a += AZ_WAVE) {
                    if (!action_legal(s, a) || rn[a] - n0[a] != want || (seen && !(rn[a] > 0.0f))) continue;
                    const double sco = b[a] + gumbel_sigma(rn[a], rw[a], sig, vmix);
                    if (bi < 0 || sco > best) {
                        best = sco;
                        bi = a;
                    }
                }
            });
        }
        const int top = Wv::argmax_first([&](int lane, double& best, int& bi) {
            for (int a = lane; a < A; a += AZ_WAVE) {
                if (!action_legal(s, a)) continue;
                const double p = (double)rp[a];
                const double logit = log(p > 1e-45 ? p : 1e-45) + gumbel_sigma(rn[a], rw[a], sig, vmix);
                sc.cdf[a] = logit;
                if (bi < 0 || logit > best) {
                    best = logit;
                    bi = a;
                }
            }
        });
        Wv::sync();
        const double mx = (top >= 0 && top < A) ? sc.cdf[top] : 0.0;
        const double sum = Wv::sum_f64([&](int lane) -> double {
            double part = 0.0;
            for (int a = lane; a < A; a += AZ_WAVE) {
                const double e = action_legal(s, a) ? exp(sc.cdf[a] - mx) : 0.0;
                sc.pi[a] = e;
                part += e;
            }
            return part;
        });
        Wv::sync();
        double* tp = m.target_pi + (size_t)g * A;
        Wv::lanes([&](int lane) {
            for (int a = lane; a < A; a += AZ_WAVE) {
                const double v = sum > 0.0 ? sc.pi[a] / sum : sc.pi[a];
                sc.pi[a] = v;
                tp[a] = v;
            }
        });
        if (Wv::first()) gr.gum_move = astar;
        Wv::sync();
        return astar;
    }
    // Gumbel mode on, but this search ran the plain rule (a fast move of the playout cap): the target row is the plain policy, no a*.
    AZ_HD void plain_target() {
        double* tp = m.target_pi + (size_t)g * A;
        Wv::lanes([&](int lane) {
            for (int a = lane; a < A; a += AZ_WAVE) tp[a] = sc.pi[a];
        });
        if (Wv::first()) gr.gum_move = -1;
        Wv::sync();
    }

    // np.random.choice(p=pi): cdf = cumsum(p) (sequential, float64), cdf /= cdf[-1], searchsorted(cdf, u, 'right').
    // The cumulative sums are formed once, in order, in LDS; fl(cdf[a] / total) is monotone in a, so the first index
    // whose quotient exceeds u is found by bisection with the very same divisions NumPy performs.
    AZ_HD int sample_move(bool warm) {
        const S& s = hdr(gr.root).st;
        if (Wv::first()) {
            double acc = 0.0;
            for (int a = 0; a < A; ++a) {
                acc += sc.pi[a];
                sc.cdf[a] = acc;
            }
        }
        Wv::sync();
        const double tot = sc.cdf[A - 1];
        const double* inj = c.inject ? m.inj_unif + ((size_t)g * c.inj_moves + (gr.ply < c.inj_moves ? gr.ply : c.inj_moves - 1)) * AZ_INJ_K : nullptr;
        int mv = -1;
        for (int t = 0; t < 64; ++t) {
            double u;
            if (c.inject) u = inj[t < AZ_INJ_K ? t : AZ_INJ_K - 1];
            else {
                u32 r[4];
                Philox::gen(c.seed + (u64)c.rank, (u32)g, (u32)gr.uid, ((u32)gr.ply << 12) | 0xFFFu, 0x1000u + (u32)t, r);
                u = Philox::u01(r[0], r[1]);
            }
            int lo = 0, hi = A;  // first a in [0, A) with cdf[a]/tot > u, else A
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (sc.cdf[mid] / tot > u) hi = mid;
                else lo = mid + 1;
            }
            mv = lo < A ? lo : A - 1;
            // mcts_v2.py:433 / :640: redraw while pass during warm-up, or illegal
            const bool bad = (warm && GAME == AZ_GO && mv == NP) || !action_legal(s, mv);
            if (!bad) return mv;
        }
        // the reference would loop forever here
        fail(AZ_ERR_SAMPLE);
        return mv;
    }

    // Policy surprise of the search that just ended (azsp_set_policy_surprise): KL(pi || P / Z) in float64, pi = the target row record_sample
    // stages (sc.pi), P = the root's prior row as the evaluator gave it (expand_node stores it unmasked; noise and the Gumbel base row live
    // in rootP), Z = its mass on the root's legal actions.  The 1e-45 floor is apply_gumbel's.
    AZ_HD float policy_surprise() {
        const S& s = hdr(gr.root).st;
        const float* rp = rowP(gr.root);
        const double z = Wv::sum_f64([&](int lane) -> double {
            double part = 0.0;
            for (int a = lane; a < A; a += AZ_WAVE)
                if (action_legal(s, a)) part += (double)rp[a];
            return part;
        });
        double kl = Wv::sum_f64([&](int lane) -> double {
            double part = 0.0;
            for (int a = lane; a < A; a += AZ_WAVE) {
                const double t = sc.pi[a];
                if (t > 0.0) {
                    const double p = (double)rp[a];
                    part += t * (log(t) - log(p > 1e-45 ? p : 1e-45));
                }
            }
            return part;
        });
        kl += z > 0.0 ? log(z) : 0.0;
        return (float)(kl > 0.0 ? kl : 0.0);
    }

    AZ_HD void record_sample(double rq) {
        int* sh = m.stg_hdr + ((size_t)g * 2 + gr.cur_buf) * SH_COUNT;
        const int k = sh[SH_LEN];
        if (k >= c.stage_cap) {
            fail(AZ_ERR_STAGE);
            return;
        }
        const size_t idx = ((size_t)g * 2 + gr.cur_buf) * c.stage_cap + k;
        u64* pl = m.stg_planes + idx * 16 * W;
        float* pi = m.stg_pi + idx * A;
        const int me = gr.env.to_play;
        float surprise = 0.0f;
        if (m.stg_surprise && c.surprise) surprise = policy_surprise();
        // observation BEFORE the move, mover's perspective (pipeline.py:323): the history ring itself
        Wv::lanes([&](int lane) {
            for (int t = lane; t < 16 * W; t += AZ_WAVE) {
                const int w = t % W, pc = t / W, kk = pc >> 1, col = (pc & 1) ? 1 - me : me;
                pl[t] = gr.hist[kk][col][w];
            }
            for (int a = lane; a < A; a += AZ_WAVE) pi[a] = (float)sc.pi[a];
        });
        if (Wv::first()) {
            m.stg_meta[idx] = (unsigned char)((me == 0 ? AZ_META_BLACK : 0) | ((gr.sim_budget & AZ_SB_FAST) ? AZ_META_FAST : 0));
            if (m.stg_rootq) m.stg_rootq[idx] = c.aux ? (float)rq : 0.0f;
            if (m.stg_surprise) m.stg_surprise[idx] = surprise;
            if (m.stg_base) m.stg_base[idx] = c.vr_L > 0 ? (float)(1.0 - vr_slot().prop * (1.0 - c.vr_w)) : 1.0f;
            sh[SH_LEN] = k + 1;
        }
        Wv::sync();
    }

    AZ_HD void push_history(const S& s) {
        // hist[k] <- hist[k-1], hist[0] <- new board (base.py deque.appendleft); 16*W words moved lane-parallel via LDS
        u64* flat = &gr.hist[0][0][0];
        Wv::lanes([&](int lane) {
            for (int t = lane; t < 16 * W; t += AZ_WAVE) {
                const int w = t % W, kq = t / W, k = kq >> 1, q = kq & 1;
                sc.planes[kq][w] = k == 0 ? s.stones[q][w] : flat[t - 2 * W];
            }
        });
        Wv::sync();
        Wv::lanes([&](int lane) {
            for (int t = lane; t < 16 * W; t += AZ_WAVE) flat[t] = sc.planes[t / W][t % W];
        });
        Wv::sync();
    }

    // Keep the subtree below `child`, return every other node to the free stack (mcts_v2.py:436-446).
    AZ_HD void reroot(int child, int mv) {
        const int old_root = gr.root;
        const float cn = rowN(old_root)[mv], cw = rowW(old_root)[mv];
        int16_t* fs = m.free_stack + (size_t)g * c.max_nodes;
        const int mn = c.max_nodes;
        const bool lds = mn <= AZ_LDS_NODES;
        // A node is kept iff walking up its parents reaches `child` before the old root.  Unused nodes carry
        // parent == -2.  The parent links are first gathered into LDS (one strided load per node, all in flight
        // together); the walks then run at LDS latency instead of one dependent global load per hop.
        if (lds) {
            for (int base = 0; base < mn; base += AZ_WAVE)
                Wv::lanes([&](int lane) {
                    const int i = base + lane;
                    if (i < mn) sc.parent[i] = hdr(i).parent;
                });
            Wv::sync();
        }
        int nfree = gr.n_free;
        for (int base = 0; base < mn; base += AZ_WAVE) {
            const u64 drop = Wv::ballot([&](int lane) -> bool {
                const int i = base + lane;
                if (i >= mn) return false;
                int p = lds ? (int)sc.parent[i] : (int)hdr(i).parent;
                if (p == -2) return false;  // not in use
                int cur = i;
                for (int hops = 0; hops < mn; ++hops) {
                    if (cur == child) return false;  // kept
                    if (cur == old_root || p < 0) return true;
                    cur = p;
                    p = lds ? (int)sc.parent[cur] : (int)hdr(cur).parent;
                }
                return true;
            });
            Wv::sync();
            Wv::lanes([&](int lane) {
                if ((drop >> lane) & 1ull) {
                    const int pos = nfree + __builtin_popcountll(drop & ((1ull << lane) - 1ull));
                    fs[pos] = (int16_t)(base + lane);
                    hdr(base + lane).parent = -2;
                    if (lds) sc.parent[base + lane] = -2;  // later walks stop here (p < 0 => dropped)
                }
            });
            nfree += __builtin_popcountll(drop);
            Wv::sync();
        }
        if (Wv::first()) {
            gr.n_free = nfree;
            gr.root = child;
            hdr(child).parent = -1;
            gr.root_N = (int)cn;  // np.float32 copies of the child's slot (mcts_v2.py:439-443)
            gr.root_W = (double)cw;
            gr.root_fresh = 0;
            gr.root_noisy = 0;
            gr.noise_pending = begin_move_class();
        }
        Wv::sync();
    }

    AZ_HD void finalize_game(const S& fin, int last_player, int resigned) {
        int* sh = m.stg_hdr + ((size_t)g * 2 + gr.cur_buf) * SH_COUNT;
        if (Wv::first()) {
            sh[SH_WINNER] = fin.winner;
            sh[SH_AREA_B] = fin.area[0];
            sh[SH_AREA_W] = fin.area[1];
            sh[SH_PASSES] = gr.num_passes;
            sh[SH_RESIGNED] = resigned;
            sh[SH_RESIGN_DISABLED] = gr.resign_disabled;
            // pipeline.py:361-365
            const int marked = (c.has_resign && gr.resign_disabled && gr.marked_player >= 0) ? 1 : 0;
            sh[SH_MARKED] = marked;
            sh[SH_COULD_WON] = (marked && fin.winner == gr.marked_player) ? 1 : 0;
            sh[SH_MARKED_PLAYER] = gr.marked_player;
            sh[SH_UID] = gr.uid;
            sh[SH_TRAINING_STEPS] = gr.train_steps;  // the weights that STARTED the game (pipeline.py:237 -> :271)
            sh[SH_TS_END] = c.training_steps;        // != the above: the game straddled a weight hot-swap
            const u64 tb = az_bits_f64(gr.resign_thr);
            sh[SH_THR_LO] = (int)(unsigned)(tb & 0xffffffffull);
            sh[SH_THR_HI] = (int)(unsigned)(tb >> 32);
            sh[SH_REWARD] = fin.reward;  // reward of `last_player` (pipeline.py:349-354 turns it into z at harvest)
            sh[SH_LAST_PLAYER] = last_player;
            sh[SH_STATE] = AZB_COMPLETE;
            gr.games_done += 1;
        }
        if (m.stg_own) {
            // auxiliary targets: who owns every point of the final position (Go: Tromp-Taylor area, whatever ended the game -- a
            // resignation leaves the board as it was; Gomoku: the stones).  One word per lane.
            B ob = O::zero(), ow = O::zero();
            if (c.aux) {
                if (GAME == AZ_GO) R::go_owner(R::ld(fin.stones[0]), R::ld(fin.stones[1]), ob, ow);
                else {
                    ob = R::ld(fin.stones[0]);
                    ow = R::ld(fin.stones[1]);
                }
            }
            u64* own = m.stg_own + ((size_t)g * 2 + gr.cur_buf) * 2 * W;
            Wv::lanes([&](int lane) {
                for (int w = 0; w < W; ++w) {
                    if (lane == w) own[w] = ob.w[w];
                    if (lane == W + w) own[W + w] = ow.w[w];
                }
            });
        }
        cnt[AZC_GAMES]++;
        Wv::sync();
    }

    // Try to start the next game in the other staging buffer; stall (AZS_WAIT_BUF) until the host harvested it.
    AZ_HD void next_game() {
        if (c.stop_at_game_end) {
            if (Wv::first()) gr.status = AZS_IDLE;
            Wv::sync();
            return;
        }
        const int other = 1 - gr.cur_buf;
        const int* sh = m.stg_hdr + ((size_t)g * 2 + other) * SH_COUNT;
        if (sh[SH_STATE] != AZB_FREE) {
            if (Wv::first()) gr.status = AZS_WAIT_BUF;
            cnt[AZC_STALLS]++;
            Wv::sync();
            return;
        }
        if (Wv::first()) gr.cur_buf = other;
        Wv::sync();
        new_game();
    }

    // ---- end of a search (mcts_v2.py:421-450) ----------------------------------------------------
    AZ_HD double root_q() const {
        if (gr.root_N <= 0) return 0.0;
        return gr.root_fresh ? gr.root_W / (double)gr.root_N : (double)((float)gr.root_W / (float)gr.root_N);
    }
    AZ_HD int log_slot() const { return c.log_moves ? (gr.ply < c.log_cap ? gr.ply : c.log_cap - 1) : 0; }
    AZ_HD double* pi_slot() const { return m.log_pi + ((size_t)g * c.log_cap + log_slot()) * A; }

    // Policy + (batched mode) move choice.  In drop-in mode (stop_after_move) the caller samples the
    // move itself from the published pi, exactly like mcts_v2.py:433-434 does with np.random.choice.
    AZ_HD void search_done() {
        const bool warm = gr.warm_override >= 0 ? (gr.warm_override != 0) : !(gr.env.steps > c.warm_up_steps);  // pipeline.py:320
        search_policy(warm, (c.log_moves || c.stop_after_move) ? pi_slot() : nullptr);
        const float* rn = rowN(gr.root);
        if (c.log_moves || c.stop_after_move) {
            float* ln = m.log_childN + ((size_t)g * c.log_cap + log_slot()) * A;
            Wv::lanes([&](int lane) {
                for (int a = lane; a < A; a += AZ_WAVE) ln[a] = rn[a];
            });
        }
        const bool gumbel = Wv::uni(gr.root_noisy) == AZ_ROOT_GUMBEL;  // this search ran the Gumbel root rule
        if (c.stop_after_move) {
            if (gumbel) gumbel_target();
            else if (c.forced_k > 0.0) make_target(warm);
            else if (c.gumbel_m > 0) plain_target();
            if (Wv::first()) {
                gr.out_root_q = root_q();
                gr.status = AZS_MOVE_DONE;
            }
            Wv::sync();
            return;
        }
        if (m.vr && c.vr_L > 0) {  // visit reduction: the history grows in front of the move choice (reroot() starts the next move)
            if (Wv::first()) vr_push(root_q());
            Wv::sync();
        }
        int mv;
        if (gumbel) {
            mv = gumbel_target();  // a* is the move, whatever warm-up and `deterministic` say; the sample records pi'
        } else if (c.deterministic) {
            mv = Wv::argmax_first([&](int lane, double& best, int& bi) {  // np.argmax(child_N), unmasked (:429)
                for (int a = lane; a < A; a += AZ_WAVE)
                    if (bi < 0 || (double)rn[a] > best) {
                        best = (double)rn[a];
                        bi = a;
                    }
            });
        } else {
            mv = sample_move(warm);
        }
        if (!gumbel && c.forced_k > 0.0) make_target(warm);  // the move came from the unpruned policy; the sample records the target
        else if (!gumbel && c.gumbel_m > 0) plain_target();
        commit_actor(mv);
    }

    // best_child_Q = -Q(chosen child) in float32 (:446); 0.0 when the move has no child node (:425)
    AZ_HD double child_q_of(int mv, int& child) const {
        child = (mv >= 0 && mv < A) ? rowC(gr.root)[mv] : -1;
        if (child < 0) return 0.0;
        const float cn = rowN(gr.root)[mv], cw = rowW(gr.root)[mv];
        return cn > 0.0f ? (double)(-(cw / cn)) : -0.0;
    }
    AZ_HD void log_outputs(int mv, double rq, double cq) {
        if (Wv::first()) {
            gr.out_move = mv;
            gr.out_root_q = rq;
            gr.out_child_q = cq;
            if (c.log_moves && gr.ply < c.log_cap) {
                double* lq = m.log_q + ((size_t)g * c.log_cap + gr.ply) * AZSP_SQ_COUNT;
                lq[AZSP_SQ_ROOT_Q] = rq;
                lq[AZSP_SQ_CHILD_Q] = cq;
                lq[AZSP_SQ_ROOT_N] = (double)gr.root_N;
                lq[AZSP_SQ_MOVE] = (double)mv;
            }
        }
        cnt[AZC_MOVES]++;
        Wv::sync();
    }

    // Drop-in uct_search: the caller steps its own env; only the tree advances (mcts_v2.py:436-446).
    AZ_HD void commit_host(int mv) {
        if (gr.status != AZS_MOVE_DONE) return;
        int child;
        const double cq = child_q_of(mv, child);
        log_outputs(mv, root_q(), cq);
        if (child >= 0 && c.reuse_tree && !(hdr(child).st.flags & AZF_TERMINAL)) {
            const S ns = hdr(child).st;
            if (Wv::first()) {
                gr.env = ns;
                gr.ply += 1;
            }
            Wv::sync();
            push_history(ns);
            reroot(child, mv);
            if (Wv::first()) gr.status = AZS_SEARCH;
        } else {
            free_all_nodes();
            if (Wv::first()) gr.status = AZS_IDLE;
        }
        if (Wv::first()) gr.noise_ready = 0;
        Wv::sync();
    }

    // Batched actor step (pipeline.py:323-346): sample, resignation rule, env step, re-root / game end.
    AZ_HD void commit_actor(int mv) {
        int child;
        const double rq = root_q();
        const double cq = child_q_of(mv, child);
        log_outputs(mv, rq, cq);
        if (child < 0) {  // cannot happen: a sampled / most-visited move always has a visited child
            fail(AZ_ERR_SAMPLE);
            if (Wv::first()) gr.status = AZS_IDLE;
            Wv::sync();
            return;
        }
        record_sample(rq);
        const int mover = gr.env.to_play;
        bool resign = false;
        if (GAME == AZ_GO && c.has_resign && gr.resign_thr > -1.0 && gr.env.steps > c.check_resign_after) {
            // root_Q is a Python float on a fresh root, np.float32 otherwise; best_child_Q is np.float32
            const double thr = gr.resign_thr;  // this game's threshold (pipeline.py:241-242, :328-333)
            const bool lo_root = gr.root_fresh ? (rq < thr) : ((float)rq < (float)thr);
            const bool lo_child = (float)cq < (float)thr;
            if (lo_root && lo_child) {
                if (gr.marked_player < 0 && Wv::first()) gr.marked_player = mover;
                Wv::sync();
                if (!gr.resign_disabled) resign = true;
            }
        }
        S ns;
        if (resign) R::go_resign(gr.env, ns);
        else ns = hdr(child).st;
        if (Wv::first()) {
            // the move that leaves the recorded position: what env.history / to_sgf() would hold (resign is not a history move)
            const int* sh = m.stg_hdr + ((size_t)g * 2 + gr.cur_buf) * SH_COUNT;
            if (sh[SH_LEN] > 0) m.stg_move[((size_t)g * 2 + gr.cur_buf) * c.stage_cap + (sh[SH_LEN] - 1)] = (int16_t)(resign ? -1 : mv);
            if (GAME == AZ_GO && !resign && mv == NP) gr.num_passes += 1;
            gr.env = ns;
            gr.ply += 1;
        }
        Wv::sync();
        push_history(ns);
        if (ns.flags & AZF_TERMINAL) {
            finalize_game(ns, mover, resign ? 1 : 0);
            next_game();
            return;
        }
        if (c.max_plies > 0 && gr.ply >= c.max_plies) {
            if (Wv::first()) gr.status = AZS_IDLE;
            Wv::sync();
            return;
        }
        if (c.reuse_tree) {
            reroot(child, mv);
        } else {
            free_all_nodes();
            if (Wv::first()) gr.status = AZS_NEED_ROOT;
            Wv::sync();
        }
    }

    // ---- one engine round for this game ---------------------------------------------------------
    AZ_HD void flush_counters() {
        if (Wv::first()) {
            u64* row = m.counters + (size_t)g * AZC_COUNT;
            for (int i = 0; i < AZC_COUNT; ++i)
                if (cnt[i]) row[i] += cnt[i];
        }
    }
    // phase A: consume the evaluator's outputs
    AZ_HD void backup_phase(const float* priors, const float* values) {
        if (Wv::uni(gr.root_eval_pending) || Wv::uni(gr.n_leaves) > 0) apply_outputs(priors, values);
    }
    // phase B: finish as many moves as the budget allows (rare per round and per game)
    AZ_HD void endmove_phase() {
        if (Wv::uni(gr.status) == AZS_WAIT_BUF) next_game();
        for (int guard = 0; guard < 8; ++guard) {
            if (Wv::uni(gr.status) != AZS_SEARCH) break;
            if (Wv::uni(gr.noise_pending) && (!c.stop_after_move || Wv::uni(gr.noise_ready))) apply_noise();
            if (Wv::uni(gr.noise_pending)) break;  // drop-in mode: the noise vector arrives with begin_move
            if (Wv::uni(gr.root_N) < game_budget()) break;
            search_done();
        }
    }
};
