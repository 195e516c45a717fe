// az_conv_sp2p.h -- k_conv3x3_sp2p<RES>: the fp32-class 3x3 convolution of the 9x9 x 128 tower (az_conv_sp.h: hi + lo f16 pairs, three
// v_mfma_f32_16x16x32_f16 products per multiply, fp32 accumulation) with a 2 x 2 SPLIT OF THE CU'S WORK BETWEEN ITS FOUR WAVES and one
// workgroup iteration per PAIR of adjacent boards (2p, 2p + 1), so that the MFMAs which only multiply the zero padding can be skipped:
//     y = relu(conv3x3(x, w) + bias [+ residual])              (alpha_zero/core/network.py:42-82, eval mode, BatchNorm folded;
//                                                               the reference evaluates in fp32: core/pipeline.py:91-123)
// The 2 x 2 split.  k_conv3x3_sp gives every wave 16 couts x all 128 cin: all four waves read EVERY B fragment of the board from LDS
// (2 reads per 3 MFMAs).  Measured (tools/probes/split_form_probe.hip, profiles/r06_split_form_probe.txt): with those reads in the loop the
// matrix cores sustain 1.50 PF/s; with half of them 1.70 PF/s.  Here wave (a, b) holds 32 couts (two 16-cout tiles) x the cin HALF b: the
// same 288 weight registers, every fragment feeds 6 MFMAs instead of 3, a wave reads half the image.
// The hand-over buffer.  The two cin halves of a cout tile meet through LDS: after a unit each wave joins (main + 2^-11 corr) the partial
// sums of the tile its PARTNER finalises, hands them over (one ds_write_b128 per column tile), and runs the epilogue of its own tile with
// the partner's partial added in.  Wave b = 1 loads its weight tiles swapped, so "own tile" is index 0 in both waves (compile-time register
// indices); the bias enters through the own tile's main accumulator only.  12 KB (3 column tiles x 4 waves x 1 KB) beside the two x images
// (120 KB) and the corner side buffer; the buffer is single, so a barrier orders a unit's hand-over writes behind the partner's reads of
// the previous hand-over.
// The riders.  A unit's MFMA stream is never interrupted: the hand-over, the finishing epilogue of the previous unit (join, residual,
// stores), the residual loads, the B-fragment requests (one ds_read_b128 per MFMA gap), the LDS-DMA pieces of the next image and the
// barriers ride in the gaps behind its MFMAs (send_op / fin_op / dma_piece below).  The finishing epilogue is the shared SpEpi of az_conv_sp.h
// with the partner add as its one extra per-element micro-op; the LDS-DMA piece is the shared sp_dma_piece with the nt policy.
// Arithmetic: result = (main_a + 2^-11 corr_a) + (main_b + 2^-11 corr_b) [+ residual]: two fp32 accumulation chains of 64 cin x 9 taps
// instead of one of 128 x 9, joined once -- fp32 round-off class (tests/test_split_tower.py bounds), not bit-identical to k_conv3x3_sp;
// k_conv3x3_spg<..., HALVES = 2> (az_conv_spg.h) repeats these chains bit for bit and runs the odd last board of a call.
// The pair.  On a 9x9 board 104 of the 729 (position, tap) pairs are off the board.  A column tile is 16 positions; inside ONE board no two
//   disjoint tiles are off the board for the same tap in all 16 positions.  Over two boards three such tiles exist: row 0 (columns 1-8), row 8
//   (columns 1-8) and column 0 (rows 0-7) of both boards: each has 3 of the 9 taps off the board = 9 of the 90 (tile, tap) pairs of a board
//   pair.  Their 6 MFMAs and 2 fragment reads per k-step are not issued: 972 MFMAs per wave and pair instead of 1080.  A skipped MFMA
//   would add exact zeros, the order of every output's sum is unchanged: bit-identical to multiplying the padding -- up to the sign of a
//   zero: a bias of exactly -0.0 turns +0 in a first padding MFMA and passes unchanged through the C operand of a later first live MFMA here.
// Tile map (sp2p_map_table, tools/gen_sp_map_pair.py): 10 column tiles per pair -- 0-2 local to board A, 3 = top edge, 4 = the same 8
// positions of both boards, 5 = bottom edge, 6 = left edge, 7-9 local to board B; the corner (8, 0) of each board stays with the
// board-batched corner phase (12 boards per batch).  A local tile is two whole board rows (columns 1-8), tile 4 one row of both boards, so that
// a tile's store fills whole write sectors (sp2p_sector_complete below).  The rows of a local tile are FOUR apart -- (1, 5), (2, 6), (3, 7), row 4
// spans -- and tiles 1, 2 are tile 0 one and two board rows lower LANE FOR LANE (sp2p_row_shifts).  A lane's lmap / omap entries carry the second
// image's LDS offset and the second board's global offset: compile-time constants, the pair is adjacent boards.
// Units (3, 2, 3, 2 column tiles; accumulator sets 0, 1, 0, 1): U0 = tiles 0-2 (image A only), U1 = tiles 3, 4,
// U2 = tiles 5-7, U3 = tiles 8, 9 (image B only).  LDS buffer 0 always holds image A, buffer 1 image B: A is free behind U2, the next pair's
// A arrives as 16 LDS-DMA pieces in U3 and is complete at U3's end barrier; B is free behind U3, this pair's B arrives in U0 and is complete
// at U0's end barrier.  Barriers per pair: 8 (per unit the hand-over barrier; the end barriers of U0 and
// U3, which also free the hand-over buffer for the next unit; U2 and U3 open with the barrier that frees it behind a unit without one).
// The MFMA slots of a unit are a compile-time list (Sp2pSched) of the live (step, column tile, weight k-step, cout tile, product) entries; the
// riders (hand-over, finishing, residual loads, fragment requests, DMA pieces, barriers) are indexed over that list.
// Shared fragments, the skewed order.  The fragment reads beside the MFMAs cost energy, and time follows energy here.  In U0 and U3
// the tiles are row shifts of one another: the B fragment of tile j at tap row dy IS the fragment of the unit's first tile at tap row j + dy.
// These units therefore walk (row set s, tap column, k-half) instead of (tap, k-half): at a step tile j multiplies its tap row s - j if that is
// -1 .. 1 -- 1, 2, 3, 2, 1 live tiles per row set in U0 (30 steps), 1, 2, 2, 1 in U3 (24 steps) -- and ONE fragment pair (hi, lo), requested in the
// first two MFMA gaps of the step before, feeds all of them.  252 fragment reads per wave and pair instead of 324; the MFMAs are the same 972,
// and every accumulator meets its weight k-steps in ascending order as before (sp2p_chains_ascend): the same chains, the same words.  U1 and
// U2 hold edge tiles and read a fragment per live tile in the plain order.
// (Measured and left out: the corner phase's two residual loads issued a unit earlier, in U3 of a corner batch's last pair -- the residual
// layer's launch became 0.4-0.7 % slower; tools/probes/make_sp_abl.py SP2P_EARLY_RES rebuilds it.)
#pragma once
#include "az_conv_sp.h"

#if defined(__HIPCC__)
#define SP2P_NB 12  // boards per corner batch (an even number: whole pairs)

// one v_fma_f32, opaque to the compiler: left to itself it pairs the four joins of a hand-over into two v_pk_fma_f32, and a packed fp32
// instruction costs about four scalar ones beside the MFMA stream (measured: profiles/r06_packed_epilogue_ab.txt)
__device__ __forceinline__ float sp2_fma_f32(float a, float s, float c) {
    float r;
    asm("v_fma_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(s), "v"(c));
    return r;
}

struct Sp2pMap {
    unsigned char cell[10 * 16];  // board * 81 + position
};
constexpr Sp2pMap sp2p_map_table = {{
    // generated by tools/gen_sp_map_pair.py (seed 66; 126 sector-complete stores): board * 81 + position of (column tile, lane & 15)
     16,  17,  48,  49,  10,  11,  12,  13,  14,  15,  46,  47,  50,  51,  52,  53,
     25,  26,  57,  58,  19,  20,  21,  22,  23,  24,  55,  56,  59,  60,  61,  62,
     34,  35,  66,  67,  28,  29,  30,  31,  32,  33,  64,  65,  68,  69,  70,  71,
      1,   2,   3,   4,  82,  83,  84,  85,  86,  87,  88,  89,   5,   6,   7,   8,
    118, 119, 120, 121,  37,  38,  39,  40,  41,  42,  43,  44, 122, 123, 124, 125,
     73,  74,  75,  76, 154, 155, 156, 157, 158, 159, 160, 161,  77,  78,  79,  80,
      0,   9,  18,  27,  81,  90,  99, 108, 117, 126, 135, 144,  36,  45,  54,  63,
     97,  98, 129, 130,  91,  92,  93,  94,  95,  96, 127, 128, 131, 132, 133, 134,
    106, 107, 138, 139, 100, 101, 102, 103, 104, 105, 136, 137, 140, 141, 142, 143,
    115, 116, 147, 148, 109, 110, 111, 112, 113, 114, 145, 146, 149, 150, 151, 152,
}};
constexpr int SP2P_NCT = 10, SP2P_KS = 18;
// tap (dy, dx) = (tap / 3 - 1, tap % 3 - 1) of position pos lies on the zero padding
constexpr bool sp2p_tap_off(int pos, int tap) {
    const int yy = pos / SpGeo9::S + tap / 3 - 1, xx = pos % SpGeo9::S + tap % 3 - 1;
    return yy < 0 || yy >= SpGeo9::S || xx < 0 || xx >= SpGeo9::S;
}
// the skip set, derived from the table: (tile, tap) is not multiplied iff the tap is off the board for all 16 positions of the tile
constexpr bool sp2p_skip(const Sp2pMap& m, int tile, int tap) {
    for (int n = 0; n < 16; ++n)
        if (!sp2p_tap_off(m.cell[tile * 16 + n] % SpGeo9::P2, tap)) return false;
    return true;
}
constexpr int sp2p_skips(const Sp2pMap& m) {
    int n = 0;
    for (int t = 0; t < SP2P_NCT; ++t)
        for (int tap = 0; tap < 9; ++tap) n += sp2p_skip(m, t, tap) ? 1 : 0;
    return n;
}
// every position of both boards but the two corners exactly once
constexpr bool sp2p_map_complete(const Sp2pMap& m) {
    bool used[2 * SpGeo9::P2] = {};
    for (int i = 0; i < SP2P_NCT * 16; ++i) {
        const int v = m.cell[i];
        if (v >= 2 * SpGeo9::P2 || v % SpGeo9::P2 == SpGeo9::CORNER || used[v]) return false;
        used[v] = true;
    }
    return true;
}
// the rule of sp_map_ok per tile (the second image lies a multiple of 256 B behind the first: same bank classes)
constexpr bool sp2p_map_conflict_free(const Sp2pMap& m) {
    for (int t = 0; t < SP2P_NCT; ++t) {
        bool bank[16] = {};
        for (int n = 0; n < 16; ++n) {
            const int r = (SpGeo9::cell_of(m.cell[t * 16 + n] % SpGeo9::P2) + ((n >= 4 && n < 12) ? 8 : 0)) & 15;
            if (bank[r]) return false;
            bank[r] = true;
        }
    }
    return true;
}
// the skip set the scheme is built on: the top edge (tile 3) has no row above, the bottom edge (tile 5) none below, the left edge (tile 6) no
// column to its left; no other (tile, tap) is skipped
constexpr bool sp2p_skips_as_designed(const Sp2pMap& m) {
    for (int t = 0; t < SP2P_NCT; ++t)
        for (int tap = 0; tap < 9; ++tap) {
            const bool want = (t == 3 && tap / 3 == 0) || (t == 5 && tap / 3 == 2) || (t == 6 && tap % 3 == 0);
            if (sp2p_skip(m, t, tap) != want) return false;
        }
    return true;
}
// 32-byte sectors of the output that ONE tile's store fills whole: neighbouring positions (p, p + 1) of a board inside a tile (a lane pair stores
// the 16 B of a position and chunk; a chunk plane is 81 x 16 B, so the pair is one sector in the chunks of one parity).  The table keeps whole
// board rows together (rows 1-7, columns 1-8: 7 pairs each, as in the two horizontal edge tiles): a line that leaves the L2 between the stores
// of two tiles is then written back in whole sectors and granules instead of twice in halves (tools/gen_sp_map_pair.py)
constexpr int sp2p_sector_complete(const Sp2pMap& m) {
    int n = 0;
    for (int t = 0; t < SP2P_NCT; ++t)
        for (int a = 0; a < 16; ++a)
            for (int b = 0; b < 16; ++b) {
                const int p = m.cell[t * 16 + a], q = m.cell[t * 16 + b];
                n += (q == p + 1 && p / SpGeo9::P2 == q / SpGeo9::P2) ? 1 : 0;
            }
    return n;
}
static_assert(sp2p_map_complete(sp2p_map_table), "pair map: every position of both boards but the two corners exactly once");
static_assert(sp2p_map_conflict_free(sp2p_map_table), "pair map: conflict-free lane groups in every tile");
static_assert(sp2p_skips_as_designed(sp2p_map_table) && sp2p_skips(sp2p_map_table) == 9, "pair map: the three edge tiles skip 3 taps each, 9 of 90 (tile, tap) pairs");
static_assert(sp2p_sector_complete(sp2p_map_table) == 126, "pair map: 9 rows of both boards in one tile each, 7 whole sectors per row");
static __device__ const Sp2pMap sp2p_map = sp2p_map_table;

// ---- the units of a pair, their steps and their live MFMA slots ------------------------------------------------------------------
constexpr int sp2p_j0(int u) { return u == 0 ? 0 : u == 1 ? 3 : u == 2 ? 5 : 8; }
constexpr int sp2p_nj(int u) { return (u & 1) ? 2 : 3; }
constexpr bool sp2p_has_end(int u) { return u == 0 || u == 3; }  // a barrier in front of the unit's last step (image complete)
// The tiles of unit u are ROW SHIFTS of its first tile: tile j0 + j is tile j0 one board row lower per j, lane for lane, and none skips a tap.
// The B fragment of tile j at tap row dy is then the LDS data of tile j0 at tap row j + dy: one read feeds every tile of the unit.
constexpr bool sp2p_row_shifts(const Sp2pMap& m, int u) {
    const int j0 = sp2p_j0(u), nj = sp2p_nj(u);
    for (int j = 0; j < nj; ++j) {
        for (int n = 0; n < 16; ++n)
            if (m.cell[(j0 + j) * 16 + n] != m.cell[j0 * 16 + n] + j * SpGeo9::S) return false;
        for (int tap = 0; tap < 9; ++tap)
            if (sp2p_skip(m, j0 + j, tap)) return false;
    }
    return true;
}
static_assert(sp2p_row_shifts(sp2p_map_table, 0) && sp2p_row_shifts(sp2p_map_table, 3), "pair map: the local tiles of a board are row shifts of one another");
static_assert(!sp2p_row_shifts(sp2p_map_table, 1) && !sp2p_row_shifts(sp2p_map_table, 2), "pair map: the units with edge tiles read a fragment per tile");
// A unit is a list of STEPS; a step is one k-half of one fragment position and has 6 MFMAs per live tile.
//   U1, U2 (a fragment per tile): step t = weight k-step t = (tap, k-half) of every tile that does not skip the tap; tile j reads its own fragment.
//   U0, U3 (row shifts, the SKEWED order): step (s, dx, k-half), row set s = -1 .. nj outermost; tile j multiplies its tap (dy, dx) = (s - j, dx)
//   where dy is in -1 .. 1, so 1, 2, 3, 2, 1 (1, 2, 2, 1) tiles are live per s, and all of them read the ONE fragment pair (hi, lo) of the step:
//   tile j0 at tap row s.  Every accumulator still meets its weight k-steps 0 .. 17 in ascending order: its chain is the one of the plain order.
constexpr int SP2P_MAXST = 6 * 5;
struct Sp2pSched {
    int n, ns;                          // live MFMA slots, steps of the unit
    bool shared;                        // one fragment pair per step (row shifts) / one per live tile
    int kstart[SP2P_MAXST + 1];         // first slot of a step
    int live_n[SP2P_MAXST];             // live column tiles of a step ...
    unsigned char live[SP2P_MAXST][3];  // ... and which (index inside the unit)
    // the fragment position of a step: tap row and column (from the (-1, -1) neighbour of tile j0 if shared, of the reading tile if not), k-half
    unsigned char frow[SP2P_MAXST], fcol[SP2P_MAXST], fkh[SP2P_MAXST];
    // per slot: step, tile, weight k-step, cout tile, product; first: the tile's first live step (accumulator initialisation)
    unsigned char st[324], jl[324], wk[324], tt[324], prod[324], first[324];
    constexpr int nfrag(int step) const { return shared ? 1 : live_n[step]; }  // fragment pairs the step reads
    constexpr int reads() const {
        int r = 0;
        for (int i = 0; i < ns; ++i) r += 2 * nfrag(i);
        return r;
    }
};
constexpr Sp2pSched sp2p_sched(int u) {
    Sp2pSched s = {};
    const int j0 = sp2p_j0(u), nj = sp2p_nj(u);
    s.shared = sp2p_row_shifts(sp2p_map_table, u);
    s.ns = s.shared ? 6 * (nj + 2) : SP2P_KS;
    int first_st[3] = {-1, -1, -1};
    int n = 0;
    for (int i = 0; i < s.ns; ++i) {
        const int row = i / 6, col = (i / 2) % 3, kh = i % 2;  // shared: row = s + 1
        int ln = 0, wk[3] = {};
        for (int j = 0; j < nj; ++j) {
            const int dy1 = s.shared ? row - j : row;  // tap row + 1 of tile j
            if (dy1 < 0 || dy1 > 2 || sp2p_skip(sp2p_map_table, j0 + j, dy1 * 3 + col)) continue;
            wk[ln] = (dy1 * 3 + col) * 2 + kh;
            s.live[i][ln++] = (unsigned char)j;
            if (first_st[j] < 0) first_st[j] = i;
        }
        s.live_n[i] = ln;
        s.kstart[i] = n;
        s.frow[i] = (unsigned char)row, s.fcol[i] = (unsigned char)col, s.fkh[i] = (unsigned char)kh;
        for (int r6 = 0; r6 < 6; ++r6)  // (cout tile, product) outer, column tile inner
            for (int k = 0; k < ln; ++k) {
                const int j = s.live[i][k];
                s.st[n] = (unsigned char)i, s.jl[n] = (unsigned char)j, s.wk[n] = (unsigned char)wk[k], s.tt[n] = (unsigned char)(r6 / 3), s.prod[n] = (unsigned char)(r6 % 3);
                s.first[n] = first_st[j] == i ? 1 : 0;
                ++n;
            }
    }
    s.kstart[s.ns] = n, s.n = n;
    return s;
}
// every tile of the unit meets each of its live weight k-steps once, in ascending order
constexpr bool sp2p_chains_ascend(const Sp2pSched& s, int u) {
    for (int j = 0; j < sp2p_nj(u); ++j)
        for (int r6 = 0; r6 < 6; ++r6) {
            int next = 0;
            for (int sl = 0; sl < s.n; ++sl) {
                if (s.jl[sl] != j || s.tt[sl] * 3 + s.prod[sl] != r6) continue;
                while (next < SP2P_KS && sp2p_skip(sp2p_map_table, sp2p_j0(u) + j, next / 2)) ++next;
                if (s.wk[sl] != next++) return false;
            }
            while (next < SP2P_KS && sp2p_skip(sp2p_map_table, sp2p_j0(u) + j, next / 2)) ++next;
            if (next != SP2P_KS) return false;
        }
    return true;
}
template <int U> struct Sp2pU {
    static constexpr Sp2pSched S = sp2p_sched(U);
    static_assert(sp2p_chains_ascend(S, U), "an accumulator's chain: its live weight k-steps, each once, ascending");
    static_assert(S.ns % 2 == 0, "the fragment ring (2 slots) is in the same phase at every unit's first step");
};
static_assert(Sp2pU<0>::S.n + Sp2pU<1>::S.n + Sp2pU<2>::S.n + Sp2pU<3>::S.n == 972, "MFMAs per wave and pair: 1080 less 9 x 12");
static_assert(Sp2pU<1>::S.n == 180, "the top tile shares its unit with the never-skipped tile");
static_assert(Sp2pU<0>::S.ns == 30 && Sp2pU<3>::S.ns == 24 && Sp2pU<0>::S.n == 324 && Sp2pU<3>::S.n == 216, "the skewed units: 1, 2, 3, 2, 1 and 1, 2, 2, 1 live tiles per row set");
static_assert(Sp2pU<0>::S.reads() == 60 && Sp2pU<1>::S.reads() == 60 && Sp2pU<2>::S.reads() == 84 && Sp2pU<3>::S.reads() == 48,
              "fragment reads per wave and pair: 252 (324 with a fragment per tile in every unit)");

// Constants of unit U's riders (shared by the kernel and by sp2p_vm_younger)
template <bool RES, int U> struct Sp2pK {
    static constexpr int NS = Sp2pU<U>::S.ns, S0 = 6, NPIECE = 16;
    // finishing micro-ops of a column tile: the partner's partial (1 read), then the epilogue with the partner add (sp_epi_* of az_conv_sp.h)
    static constexpr int PAIR = sp_epi_pair(RES, true), CT_OPS = sp_epi_ct_ops(RES, true), P2CT = CT_OPS + 1;
    static constexpr int PU = (U + 3) & 3, NU = (U + 1) & 3;
    static constexpr int nj = sp2p_nj(U), j0 = sp2p_j0(U), pnj = sp2p_nj(PU), pj0 = sp2p_j0(PU);
    static constexpr bool END = sp2p_has_end(U), PRE = !sp2p_has_end(PU);
    static constexpr int N = Sp2pU<U>::S.n, KLAST = Sp2pU<U>::S.kstart[NS - 1];  // KLAST: first slot of the last step
    static constexpr int P1 = 5 * pnj, SBX = S0 + P1 + 1, P2 = pnj * P2CT;
    static constexpr int AVAIL = (END ? KLAST : N - 4) - (SBX + 1);
    typedef SpSpread<P2, SBX + 1, AVAIL> SP;
    // the LDS-DMA pieces of the unit (U0: this pair's image B, U3: the next pair's image A): piece k behind slot PFIRST + k PSTRIDE, early in the
    // unit -- the image is needed at the unit's end barrier
    static constexpr bool DMA = END;
    static constexpr int PFIRST = SBX + 3, PSTRIDE = U == 0 ? 9 : 6, PLAST = PFIRST + (NPIECE - 1) * PSTRIDE;
    static_assert(SP::MAXPER <= 1, "the previous unit's finishing fits this unit's MFMA gaps");
    static_assert(SBX + 1 < Sp2pU<U>::S.kstart[4] && 2 * nj <= S0, "hand-over early in the unit; residual loads in front of it");
    static_assert(!DMA || (PLAST + 2 * 6 * nj < KLAST && PFIRST > SBX), "pieces behind the barrier that frees the image, well in front of the end barrier");
};
// Vector-memory instructions a wave issues between the last LDS-DMA piece of unit U and the unit's end barrier: the stores of the finishing
// riders behind the last piece (2 per column tile are the last two micro-ops of a tile); the residual loads are older than the first piece.
template <bool RES, int U> __host__ __device__ constexpr int sp2p_vm_younger() {
    typedef Sp2pK<RES, U> K;
    return sp_epi_stores_behind<typename K::SP>(K::pnj, K::P2CT, 1, K::PLAST);
}

template <bool RES> __global__ void __launch_bounds__(CW_THREADS, 1)
k_conv3x3_sp2p(const unsigned char* __restrict__ x, const _Float16* __restrict__ w, const float* __restrict__ bias,
               const unsigned char* __restrict__ res, unsigned char* __restrict__ y, int npairs, int relu, unsigned* range) {
    typedef SpGeo9 G;
    constexpr int C = 128, CIN = 128, NCH = 16, NCG = 2;
    constexpr int KSUB = 2, KS = SP2P_KS;
    constexpr int NT = 2;
    constexpr int NJ0 = 3, NJ1 = 2, R = 2;
    constexpr int LBLK = G::CELLS * 16, LPLANE = NCH * LBLK, LBUF = 2 * LPLANE;
    constexpr int GBLK = G::P2 * 16, XPLANE = NCH * GBLK, XTILE = 2 * XPLANE;
    constexpr int YPLANE = (C / 8) * GBLK, YTILE = 2 * YPLANE;
    constexpr int NP = (G::CELLS + 63) / 64, SPW = 2 * NCH / 4, NPIECE = NP * SPW;
    constexpr int NF = NT * 2 * KS;
    constexpr int NF_A = 64;
    constexpr int P2CT = Sp2pK<RES, 0>::P2CT, PAIR = Sp2pK<RES, 0>::PAIR, S0 = Sp2pK<RES, 0>::S0;
    static_assert(NPIECE == Sp2pK<RES, 0>::NPIECE && KS % R == 0, "pieces per image; ring phase");
    constexpr int SIDE_BOARD = 8 * NCH * 16 + 16, SIDE0 = 2 * LBUF + 16, XB0 = SIDE0 + SP2P_NB * SIDE_BOARD, XBCT = 4 * 1024;
    __shared__ __attribute__((aligned(1024))) unsigned char lds[XB0 + NJ0 * XBCT];
    static_assert(XB0 + NJ0 * XBCT <= 160 * 1024 && XB0 % 16 == 0, "LDS budget");
    const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, kg = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wa = wave >> 1, wb = wave & 1;
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)lds;
    int cg, slot, nslot;
    sp_wg_map(NCG, cg, slot, nslot);
    for (int i = tid; i < (XB0 + NJ0 * XBCT) / 16; i += CW_THREADS) *(cv_u32x4*)(lds + i * 16) = (cv_u32x4){0u, 0u, 0u, 0u};
    CV_BARRIER();
    if (slot >= npairs) return;

    // A fragments of tile index tt = cout tile (tt + b) & 1 of the wave pair's 32 couts, cin half b
    sp_f16x8 wf[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        const int tt = f / (2 * KS), pl = (f / KS) & 1, st = f % KS;
        wf[f] = *(const sp_f16x8*)(w + ((size_t)((pl * 9 + st / KSUB) * C + cg * 64 + wa * 32 + ((tt + wb) & 1) * 16 + l15)) * CIN + wb * 64 + (st % KSUB) * 32 + kg * 8);
    }
    c6_f32x4 bv;  // bias of the OWN tile in the D layout
#pragma unroll
    for (int e = 0; e < 4; ++e) bv[e] = bias[cg * 64 + wa * 32 + wb * 16 + 4 * kg + e];
    const float lo_relu = relu ? 0.0f : -__builtin_inff();
    const float lo_clamp = relu ? 0.0f : -SP_F16_MAX;

    unsigned dsrc[NP];
    unsigned long long dmask[NP];
    sp_dma_plan(dsrc, dmask, lane, [](int cell) { return cell < G::CELLS ? G::pos_of_cell(cell) * 16 : -1; });
    auto dma_piece = [&](const unsigned char* src, unsigned dstbuf, bool live, int i) {
        // nt: the image is read by this workgroup and by the one of the other cout group on the same XCD at about the same time, then never again;
        // as streaming lines it stops pushing the half-written output lines out of the L2 (fewer bytes written, the same bytes fetched: DESIGN 3.1)
        sp_dma_piece<true>(src, dstbuf, SPW * wave + i / NP, i % NP, GBLK, LBLK, live ? dmask[i % NP] : 0ull, dsrc[i % NP]);
    };
    // per lane and column tile: LDS offset of the (-1, -1) neighbour in the image of the position's board (image B = + LBUF), this lane's group
    // of the wave's cin half; offset of the lane's 8-byte output slot from the pair's base (board B = + YTILE)
    unsigned lmap[SP2P_NCT], omap[SP2P_NCT];
#pragma unroll
    for (int j = 0; j < SP2P_NCT; ++j) {
        const int v = sp2p_map.cell[j * 16 + l15], bd = v >= G::P2 ? 1 : 0, pos = v - bd * G::P2;
        lmap[j] = (unsigned)(bd * LBUF + (G::PITCH * (pos / G::S) + pos % G::S) * 16 + kg * LBLK + wb * (8 * LBLK));
        omap[j] = (unsigned)(bd * YTILE + pos * 16 + (kg >> 1) * GBLK + (kg & 1) * 8);
    }
    auto out_off = [&](int j) __attribute__((always_inline)) {
        unsigned v = omap[j];
        asm volatile("" : "+v"(v));
        return v;
    };
    sp_f16x8 bb[R][2][NJ0];
    // request q of step lt of unit lu: plane q / nfrag of the step's fragment q % nfrag, into ring slot lt % R.  A skewed unit keeps its one
    // fragment per step in the ring registers of its first tile and addresses it from that tile's lmap entry
    auto frag_req = [&](auto LU, auto LT, auto QC) __attribute__((always_inline)) {
        constexpr int lu = decltype(LU)::value, lt = decltype(LT)::value, q = decltype(QC)::value;
        constexpr int nf = Sp2pU<lu>::S.nfrag(lt), pl = q / nf;
        constexpr int jr = Sp2pU<lu>::S.shared ? 0 : Sp2pU<lu>::S.live[lt][q % nf];
        constexpr int off = (Sp2pU<lu>::S.frow[lt] * G::PITCH + Sp2pU<lu>::S.fcol[lt]) * 16 + Sp2pU<lu>::S.fkh[lt] * (4 * LBLK);
        static_assert(pl < 2, "two planes per fragment");
        bb[lt % R][pl][jr] = *(const sp_f16x8*)(lds + lmap[sp2p_j0(lu) + jr] + off + pl * LPLANE);
    };
    {
        const unsigned char* src = x + (size_t)slot * (2 * XTILE);  // image A of the first pair; its image B rides in U0
#pragma unroll
        for (int i = 0; i < NPIECE; ++i) dma_piece(src, lds0, true, i);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        CV_BARRIER();
        static_assert(Sp2pU<0>::S.nfrag(0) == 1, "the first step of a pair reads one fragment");
        frag_req(CpInt<0>{}, CpInt<0>{}, CpInt<0>{});
        frag_req(CpInt<0>{}, CpInt<0>{}, CpInt<1>{});
    }
    sp_pin_a<NF_A>(wf);
    asm volatile("" : : "v"(bv), "v"(lmap[0]), "v"(lmap[SP2P_NCT - 1]), "v"(dsrc[0]), "v"(dsrc[NP - 1]));

    c6_f32x4 accm[2][NJ0][NT] = {}, accc[2][NJ0][NT] = {};  // [accumulator set][column tile of the unit][cout tile]
    cv_u32x2 rr[2][NJ0][2] = {};                            // residual of the own tile: [set][column tile][plane]
    SpEpi ep;
    c6_f32x4 xs = (c6_f32x4){0.0f, 0.0f, 0.0f, 0.0f}, xr = (c6_f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    unsigned char* const xb_mine = lds + XB0 + wave * 1024 + lane * 16;
    const unsigned char* const xb_partner = lds + XB0 + (wave ^ 1) * 1024 + lane * 16;
    // hand-over micro-op o of column tile c of the unit with accumulator set `set`: join the partner's tile (4), write it (1)
    auto send_op = [&](int set, int c, int o) {
        if (o < 4) xs[o] = sp2_fma_f32(accc[set][c][1][o], SP_INV_SCALE, accm[set][c][1][o]);
        else *(c6_f32x4*)(xb_mine + c * XBCT) = xs;
    };
    // micro-op o of the finishing of column tile c (table index mj): the partner's partial (1 read), then the epilogue of the own tile
    auto fin_op = [&](int set, int c, int mj, const SpOut& out, int o, bool store_ok) {
        if (o == 0) xr = *(const c6_f32x4*)(xb_partner + c * XBCT);
        else if (o - 1 < 2 * PAIR) ep.op<RES, true>(o - 1, accm[set][c][0], accc[set][c][0], rr[set][c], lo_clamp, &xr);
        else ep.store(o - 1 - 2 * PAIR, out, out_off(mj), store_ok);
    };

    const bool copier = tid < 8 * NCH;
    int csrc, cdst;
    {
        constexpr int KF = NCH / 4;  // k-steps of 32 over all 128 input channels (the side buffer holds both halves)
        const int c = copier ? tid : 0, ks = c % KF, pl = (c / KF) & 1, tp = (c / (2 * KF)) & 3, g4 = c / (8 * KF);
        csrc = (pl * NCH + 4 * ks + g4) * LBLK + (G::CELL0 + G::PITCH * (G::S - 2 + (tp >> 1)) + (tp & 1)) * 16;
        cdst = SIDE0 + c * 16;
    }
    cv_u32x4 ctmp = (cv_u32x4){0u, 0u, 0u, 0u};

    int it = 0, cb = 0;  // cb: boards in the corner side buffer
    SpOut yprev = {y, (sp_gptr)(unsigned long long)y};
    for (int pair = slot; pair < npairs; pair += nslot, ++it) {
        const bool has_next = pair + nslot < npairs;
        const unsigned char* bsrc = x + (size_t)pair * (2 * XTILE) + XTILE;                                  // this pair's image B
        const unsigned char* nsrc = x + (size_t)(has_next ? pair + nslot : pair) * (2 * XTILE);              // the next pair's image A
        const size_t yo = (size_t)pair * (2 * YTILE) + (size_t)(cg * 8 + wa * 4 + wb * 2) * GBLK;  // the own tile's two chunk strips, board A
        const SpOut rbase = sp_out_base(RES ? res + yo : y + yo, YPLANE), ybase = sp_out_base(y + yo, YPLANE);
        const bool have_prev = it > 0;
        auto unit = [&](auto UC) __attribute__((always_inline)) {
            constexpr int u = decltype(UC)::value, set = u & 1, pset = set ^ 1;
            typedef Sp2pK<RES, u> K;
            typedef typename K::SP SP;
            constexpr int nj = K::nj, j0 = K::j0, pj0 = K::pj0;
            const SpOut pout = u == 0 ? yprev : ybase;
            const bool pstore = u > 0 || have_prev;
            cp_for_each([&](auto SC) __attribute__((always_inline)) {
                constexpr int sl = decltype(SC)::value;  // MFMA slot of the unit
                constexpr int t = Sp2pU<u>::S.st[sl], jl = Sp2pU<u>::S.jl[sl], wk = Sp2pU<u>::S.wk[sl], tt = Sp2pU<u>::S.tt[sl], prod = Sp2pU<u>::S.prod[sl];
                constexpr int jb = Sp2pU<u>::S.shared ? 0 : jl;  // the ring registers of the slot's fragment: of its tile, or the step's one fragment
                constexpr int qi = sl - Sp2pU<u>::S.kstart[t];
                constexpr bool first = Sp2pU<u>::S.first[sl] != 0;
                if constexpr (K::END && sl == K::KLAST) {
                    // the image that arrived in this unit is complete: this wave's pieces are older than the VM_YOUNGER youngest vector-memory
                    // instructions it has issued (finishing stores), which may stay in flight.  Every wave has issued its reads of the image that
                    // the next unit's pieces overwrite, and has read the hand-over that the next unit's hand-over overwrites.
                    constexpr int VM_YOUNGER = sp2p_vm_younger<RES, u>();
                    static_assert(VM_YOUNGER < 63, "vmcnt field");
                    if (pstore) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(VM_YOUNGER) : "memory");
                    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // first pair: U0's finishing stores were not issued
                    CV_BARRIER();
                }
                if constexpr (K::PRE && sl == S0 - 1) CV_BARRIER();  // every wave has finished the previous unit: its reads of the hand-over (and of image A)
                if constexpr (sl == K::SBX) CV_BARRIER();             // the hand-over writes of all waves are in LDS
                constexpr int fa = (tt * 2 + (prod == 2 ? 1 : 0)) * KS + wk, pl = prod == 1 ? 1 : 0;
                static_assert(!first || fa < NF_A, "an accumulator's first MFMA reads its weights from the AGPRs");
                if constexpr (prod == 0) {
                    if constexpr (first && tt == 0) sp_mfma_ac(accm[set][jl][tt], wf[fa], bb[t % R][pl][jb], bv);
                    else if constexpr (first) sp_mfma_a0(accm[set][jl][tt], wf[fa], bb[t % R][pl][jb]);
                    else if constexpr (fa < NF_A) sp_mfma_a(accm[set][jl][tt], wf[fa], bb[t % R][pl][jb]);
                    else sp_mfma_v(accm[set][jl][tt], wf[fa], bb[t % R][pl][jb]);
                } else if constexpr (prod == 1) {
                    if constexpr (first) sp_mfma_a0(accc[set][jl][tt], wf[fa], bb[t % R][pl][jb]);
                    else if constexpr (fa < NF_A) sp_mfma_a(accc[set][jl][tt], wf[fa], bb[t % R][pl][jb]);
                    else sp_mfma_v(accc[set][jl][tt], wf[fa], bb[t % R][pl][jb]);
                } else {
                    if constexpr (fa < NF_A) sp_mfma_a(accc[set][jl][tt], wf[fa], bb[t % R][pl][jb]);
                    else sp_mfma_v(accc[set][jl][tt], wf[fa], bb[t % R][pl][jb]);
                }
                {   // the fragments of the next step (of this unit, or step 0 of the next unit), one request per MFMA gap
                    constexpr bool lsame = t + 1 < K::NS;
                    constexpr int lu = lsame ? u : K::NU, lt = lsame ? t + 1 : 0;
                    constexpr int nreq = 2 * Sp2pU<lu>::S.nfrag(lt);
                    static_assert(nreq <= 6 * Sp2pU<u>::S.live_n[t], "a fragment per MFMA gap");
                    if constexpr (qi < nreq) frag_req(CpInt<lu>{}, CpInt<lt>{}, CpInt<qi>{});
                }
                if constexpr (sl >= S0 && sl < S0 + K::P1) send_op(pset, (sl - S0) / 5, (sl - S0) % 5);
                if constexpr (sl > K::SBX) {
                    constexpr int o = SP::cum(sl - 1);
                    if constexpr (o < SP::cum(sl)) fin_op(pset, o / P2CT, pj0 + o / P2CT, pout, o % P2CT, pstore);
                }
                if constexpr (RES && sl < 2 * nj) {  // this unit's residual of the own tile (used by its finishing inside the next unit)
                    constexpr int rj = sl >> 1, rp = sl & 1;
                    rr[set][rj][rp] = sp_load8(rbase, rp, out_off(j0 + rj));
                }
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (K::DMA && sl >= K::PFIRST && sl <= K::PLAST && (sl - K::PFIRST) % K::PSTRIDE == 0) {
                    if constexpr (u == 0) dma_piece(bsrc, lds0 + LBUF, true, (sl - K::PFIRST) / K::PSTRIDE);
                    else dma_piece(nsrc, lds0, has_next, (sl - K::PFIRST) / K::PSTRIDE);
                    __builtin_amdgcn_sched_barrier(0);
                }
                // the corner cells of board A (U0) / board B (U2: its image is complete since U0's end barrier) -> side buffer
                if constexpr ((u == 0 || u == 2) && sl == Sp2pU<u>::S.kstart[3] - 1) {
                    if (copier) ctmp = *(const cv_u32x4*)(lds + csrc + (u == 2 ? LBUF : 0));
                    __builtin_amdgcn_sched_barrier(0);
                }
                if constexpr ((u == 0 || u == 2) && sl == Sp2pU<u>::S.kstart[6] - 1) {
                    if (copier) *(cv_u32x4*)(lds + cdst + (cb + (u == 2 ? 1 : 0)) * SIDE_BOARD) = ctmp;
                    __builtin_amdgcn_sched_barrier(0);
                }
            }, typename CpMakeSeq<K::N>::type{});
        };
        unit(CpInt<0>{});
        unit(CpInt<1>{});
        unit(CpInt<2>{});
        unit(CpInt<3>{});
        yprev = ybase;
        cb += 2;
        if (cb == SP2P_NB || !has_next) {
            // ---- the corner (8, 0) of the last cb boards: [2 x 16 couts] x [<= 12 boards] x [4 taps x this wave's 64 cin] per wave, then the hand-over
            const int n_ok = cb, it0 = it - (cb / 2 - 1);
            c6_f32x4 cm[NT], cc[NT];
            constexpr int KF = NCH / 4;
            const unsigned char* sb = lds + SIDE0 + l15 * SIDE_BOARD + kg * (8 * KF * 16);
            const int nb = l15 < n_ok ? l15 : 0;
            const size_t board = 2 * ((size_t)slot + (size_t)(it0 + (nb >> 1)) * nslot) + (nb & 1);
            const size_t co = board * YTILE + (size_t)(cg * 8 + wa * 4 + wb * 2 + (kg >> 1)) * GBLK + G::CORNER * 16 + (kg & 1) * 8;
            if (RES) {
                rr[0][0][0] = *(const cv_u32x2*)(res + co);
                rr[0][0][1] = *(const cv_u32x2*)(res + co + YPLANE);
            }
            cp_for_each([&](auto TC) __attribute__((always_inline)) {
                constexpr int u = decltype(TC)::value, tp = u / KSUB, ks = u % KSUB;
                constexpr int fw = ((tp >> 1) * 3 + 1 + (tp & 1)) * KSUB + ks;  // weight k-step of tap (dy, dx) = (tp / 2 - 1, tp % 2)
                const sp_f16x8 bh = *(const sp_f16x8*)(sb + ((tp * 2 + 0) * KF + wb * KSUB + ks) * 16);
                const sp_f16x8 bl = *(const sp_f16x8*)(sb + ((tp * 2 + 1) * KF + wb * KSUB + ks) * 16);
#pragma unroll
                for (int tt = 0; tt < NT; ++tt) {
                    const int fh = (tt * 2 + 0) * KS + fw, fl = (tt * 2 + 1) * KS + fw;
                    if (u == 0 && tt == 0) sp_mfma_ac(cm[tt], wf[fh], bh, bv);
                    else if (u == 0) sp_mfma_a0(cm[tt], wf[fh], bh);
                    else if (fh < NF_A) sp_mfma_a(cm[tt], wf[fh], bh);
                    else sp_mfma_v(cm[tt], wf[fh], bh);
                    if (u == 0) sp_mfma_a0(cc[tt], wf[fh], bl);
                    else if (fh < NF_A) sp_mfma_a(cc[tt], wf[fh], bl);
                    else sp_mfma_v(cc[tt], wf[fh], bl);
                    if (fl < NF_A) sp_mfma_a(cc[tt], wf[fl], bh);
                    else sp_mfma_v(cc[tt], wf[fl], bh);
                }
                __builtin_amdgcn_sched_barrier(0);
            }, typename CpMakeSeq<4 * KSUB>::type{});
            asm volatile("s_nop 15\n\ts_nop 15" : "+v"(cm[0]), "+v"(cc[0]), "+v"(cm[1]), "+v"(cc[1]));
            c6_f32x4 hs;
#pragma unroll
            for (int e = 0; e < 4; ++e) hs[e] = fmaf(cc[1][e], SP_INV_SCALE, cm[1][e]);
            *(c6_f32x4*)(xb_mine) = hs;
            CV_BARRIER();
            const c6_f32x4 hr = *(const c6_f32x4*)(xb_partner);
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaf(cc[0][e], SP_INV_SCALE, cm[0][e]) + hr[e];
            if (RES) {
                const cv_u32x2 rh = rr[0][0][0], rl = rr[0][0][1];
                v[0] += sp_join(sp_lo16(rh.x), sp_lo16(rl.x));
                v[1] += sp_join(sp_hi16(rh.x), sp_hi16(rl.x));
                v[2] += sp_join(sp_lo16(rh.y), sp_lo16(rl.y));
                v[3] += sp_join(sp_hi16(rh.y), sp_hi16(rl.y));
            }
            _Float16 h[4], l[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (l15 < n_ok) ep.mx = fmaxf(ep.mx, fabsf(v[e]));
                v[e] = fmaxf(v[e], lo_relu);
                sp_split(v[e], h[e], l[e]);
            }
            if (l15 < n_ok) {
                *(cv_u32x2*)(y + co) = (cv_u32x2){sp_pack(h[0], h[1]), sp_pack(h[2], h[3])};
                *(cv_u32x2*)(y + co + YPLANE) = (cv_u32x2){sp_pack(l[0], l[1]), sp_pack(l[2], l[3])};
            }
            cb = 0;
            CV_BARRIER();  // the next batch's copies may overwrite the side buffer, the next hand-over the buffer
        }
    }
    // the very last unit (accumulator set 1, board B's last two local tiles): hand over, meet, finish
    asm volatile("s_nop 15\n\ts_nop 15" : "+v"(accm[1][0][0]), "+v"(accm[1][1][0]), "+v"(accc[1][0][0]), "+v"(accc[1][1][0]), "+v"(accm[1][0][1]), "+v"(accm[1][1][1]),
                 "+v"(accc[1][0][1]), "+v"(accc[1][1][1]));
#pragma unroll
    for (int c = 0; c < NJ1; ++c)
#pragma unroll
        for (int o = 0; o < 5; ++o) send_op(1, c, o);
    CV_BARRIER();
#pragma unroll
    for (int c = 0; c < NJ1; ++c)
#pragma unroll
        for (int o = 0; o < P2CT; ++o) fin_op(1, c, sp2p_j0(3) + c, yprev, o, true);
    sp_range_report(ep.mx, range);
}
#endif  // __HIPCC__
