// az_stem_spg.h -- the stem of the fp32-class evaluator with one WAVE per output tile: k_conv3x3_spg (az_conv_spg.h) for the stem's geometry.
// (A header of its own: the text of az_conv_spg.h is what the counter summaries of the tower kernels are keyed to, tools/kernel_digest.py.)
#pragma once
#include "az_conv_spg.h"

#if defined(__HIPCC__)
// The STEM of the fp32-class evaluator for ANY board (azsp_stem_split on shapes without a tailored stem, and on a handful of boards):
//     y = relu(conv3x3(x, w, padding = pad) + bias)
// x: the split features [board][plane: hi, lo][4 chunks][n*n positions][8 channels] f16 (32 channels: azsp_split_features / the engine's
// AZSP_FEAT_F16_SPLIT), w: [2][9][C][32] f16, y: the split layout on S x S planes, S = n + 2 (pad - 1) -- a pad-3 convolution of the board is
// the pad-1 convolution of the board embedded at (off, off) = (pad - 1, pad - 1) of the zero S x S plane.  This is k_conv3x3_spg with KSUB = 1
// (nine k-steps, one per tap, K = the 32 padded input channels) and the INPUT geometry separate from the output's: output position (r, c)
// reads input cell (r + dy - off, c + dx - off); a cell outside [0, n)^2 -- plane border or embedding margin -- is a zero fragment (the load
// is redirected to cell 0 of the lane's own board, the result replaced by zeros).
// The chains of the tailored stems (k_conv3x3_sp / _sp17 with NCH = 4), hence the same bits: main = bias, then w_hi x_hi for taps 0 .. 8;
// corr = w_hi x_lo, then w_lo x_hi per tap; v = fma(corr, 2^-11, main).  XLO0 (the _exact entry: 0 / 1 planes, lo plane never written): no
// lo loads, no w_hi x_lo product.
// Dead lanes of a partial column tile start from a zero accumulator instead of the bias and multiply zero fragments only: they compute an
// exact 0, which neither stores (live[]) nor reaches the range record.
// ONE instantiation, (NT, NJ) = (1, 2), the tower's latency tile, for small and large calls alike: a wave is 54 MFMAs behind 54 fragment
// loads, so a stem is 1 / (2 KSUB) of one tower convolution's matrix work (1/4 at 64 filters, 1/16 at 256) and a network has two of those per
// block; a second, larger tile would buy at most a third of the stem's L1 traffic ((NT + NJ) / (3 NT NJ) KB per MFMA: 1 -> 0.67 at (2, 2))
// for twice the waves' latency on one board, where the stem's launch is a fixed cost of every small forward.  The small-call count of
// azsp_small_batch_waves is then exactly this kernel's wave count.
template <bool XLO0, int NT, int NJ, int R = 3> __global__ void __launch_bounds__(256)
k_stem_spg(const unsigned char* __restrict__ x, const _Float16* __restrict__ w, const float* __restrict__ bias, unsigned char* __restrict__ y, int nboards,
           int n, int off, int C, int relu, unsigned* range) {
    constexpr int CIN = 32, NST = 9;
    static_assert(NST >= R, "k-steps");
    const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, kg = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int S = n + 2 * off, P2 = S * S, PI = n * n, NCT = (P2 + 15) >> 4, NJG = (NCT + NJ - 1) / NJ, NCG = C / (16 * NT);
    const long long item = (long long)blockIdx.x * 4 + wave;
    if (item >= (long long)nboards * NJG * NCG) return;  // (uniform per wave; the kernel has no barrier)
    const int cg = (int)(item % NCG), jg = (int)((item / NCG) % NJG);
    const long long board = item / ((long long)NCG * NJG);
    const size_t xplane = (size_t)4 * PI * 16, yplane = (size_t)(C / 8) * P2 * 16;
    const unsigned char* xb = x + (size_t)board * 2 * xplane + (size_t)kg * PI * 16;
    const _Float16* wb = w + (size_t)(cg * NT * 16 + l15) * CIN + kg * 8;

    int pos[NJ], src0[NJ];  // output position; input cell of the centre tap (may lie outside the board: only used under its `inside` bit)
    unsigned inside[NJ];    // bit tap: the tap's source cell is on the board
    bool live[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int p = (jg * NJ + j) * 16 + l15;
        live[j] = p < P2;
        pos[j] = live[j] ? p : P2 - 1;
        const int r = pos[j] / S - off, c = pos[j] % S - off;
        src0[j] = r * n + c;
        unsigned m = 0;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int yy = r + tap / 3 - 1, xx = c + tap % 3 - 1;
            m |= (yy >= 0 && xx >= 0 && yy < n && xx < n) ? (1u << tap) : 0u;
        }
        inside[j] = live[j] ? m : 0u;
    }
    sp_f16x8 ra[R][2][NT], rb[R][2][NJ];  // the ring: [k-step slot][plane][tile]
    auto load_step = [&](int tap, int slot) __attribute__((always_inline)) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            ra[slot][0][t] = *(const sp_f16x8*)(wb + ((size_t)tap * C + t * 16) * CIN);
            ra[slot][1][t] = *(const sp_f16x8*)(wb + ((size_t)(9 + tap) * C + t * 16) * CIN);
        }
        const int d = (tap / 3 - 1) * n + (tap % 3 - 1);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int q = ((inside[j] >> tap) & 1u) ? src0[j] + d : 0;
            const unsigned char* src = xb + (size_t)q * 16;
            rb[slot][0][j] = *(const sp_f16x8*)src;
            if constexpr (!XLO0) rb[slot][1][j] = *(const sp_f16x8*)(src + xplane);
        }
    };
    c6_f32x4 am[1][NT][NJ], ac[1][NT][NJ];
    const float lo_clamp = relu ? 0.0f : -SP_F16_MAX;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        c6_f32x4 bv;
#pragma unroll
        for (int e = 0; e < 4; ++e) bv[e] = bias[(cg * NT + t) * 16 + 4 * kg + e];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            am[0][t][j] = live[j] ? bv : (c6_f32x4){0.0f, 0.0f, 0.0f, 0.0f};
            ac[0][t][j] = (c6_f32x4){0.0f, 0.0f, 0.0f, 0.0f};
        }
    }
#pragma unroll
    for (int s = 0; s < R - 1; ++s) load_step(s, s);
    cp_for_each([&](auto SC) __attribute__((always_inline)) {
        constexpr int tap = decltype(SC)::value, slot = tap % R;
        if constexpr (tap + R - 1 < NST) load_step(tap + R - 1, (tap + R - 1) % R);
        __builtin_amdgcn_sched_barrier(0);
        const sp_f16x8 zero = (sp_f16x8){0, 0, 0, 0, 0, 0, 0, 0};
        sp_f16x8 bh[NJ], bl[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const bool in = (inside[j] >> tap) & 1u;
            bh[j] = in ? rb[slot][0][j] : zero;
            if constexpr (!XLO0) bl[j] = in ? rb[slot][1][j] : zero;
        }
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                am[0][t][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ra[slot][0][t], bh[j], am[0][t][j], 0, 0, 0);
                if constexpr (!XLO0) ac[0][t][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ra[slot][0][t], bl[j], ac[0][t][j], 0, 0, 0);
                ac[0][t][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ra[slot][1][t], bh[j], ac[0][t][j], 0, 0, 0);
            }
        __builtin_amdgcn_sched_barrier(0);
    }, typename CpMakeSeq<NST>::type{});

    spg_epilogue<false, NT, NJ, 1>(am, ac, pos, live, nullptr, y, board, yplane, P2, cg, kg, lo_clamp, range);
}
#endif
