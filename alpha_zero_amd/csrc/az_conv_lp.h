// az_conv_lp.h -- what the lower-precision (bf16 / f16 activations, one rounding per output) weight-stationary tower kernels share.  Today
// its users are k_conv3x3_t64 and k_resblock64 (az_conv64.h); k_conv3x3_hb19 and k_conv3x3_op19q (az_conv19.h) still carry their own copies of
// the same pieces and move here together with a fresh counter pass of their family (their header is hashed into profiles/conv19_kernel_pmc.json).
// The unit schedules, map placement policies, bias layouts and MFMA wrappers differ and stay in the kernels; the pieces they issue are these.
// Two things are deliberately NOT merged here:
//   * k_conv3x3_tiled (az_conv.h) keeps its own copy of the DMA piece and of the epilogue arithmetic: az_conv.h is hashed into every
//     counter summary under profiles/, and this header includes az_conv.h, not the other way round.
//   * lp_dma_piece / lp_dma_plan / lp_pin_a sit BESIDE sp_dma_piece / sp_dma_plan / sp_pin_a (az_conv_sp.h) and repeat them: az_conv_sp.h
//     includes az_conv64.h, so the 64-filter kernels cannot include it back, and its text is hashed into the fp32-class summaries as well.
//     Whoever re-collects those counters next can fold the two copies into one.
#pragma once
#include "az_conv.h"

#if defined(__HIPCC__)
typedef __attribute__((ext_vector_type(4))) float lp_f32x4;

// ---- column-tile maps (compile-time) ----------------------------------------------------------------------------------------------
// A service group = the 16 lanes of one ds_read_b128 pass; its 16 cells must lie on 16 distinct bank residues (cell mod 16).
// The unused slots of a group: for every residue it lacks, the first position p < npos whose cell has it -> put(slot, p).
template <class CellOf, class Put> constexpr void lp_map_fill(int& fill, bool (&used)[16], int npos, CellOf cell_of, Put put) {
    for (int r = 0; r < 16 && fill < 16; ++r) {
        if (used[r]) continue;
        for (int p = 0; p < npos; ++p)
            if ((cell_of(p) & 15) == r) {
                put(fill++, p);
                used[r] = true;
                break;
            }
    }
}
// A group is conflict-free: 16 slots, and the cells cell_at(i) (< 0: a slot that does not count) on distinct residues.
template <class CellAt> constexpr bool lp_group_ok(int fill, CellAt cell_at) {
    bool seen[16] = {}, ok = fill == 16;
    for (int i = 0; i < 16; ++i) {
        const int c = cell_at(i);
        if (c < 0) continue;
        if (seen[c & 15]) ok = false;
        seen[c & 15] = true;
    }
    return ok;
}

// ---- set-up pieces ----------------------------------------------------------------------------------------------------------------
// Zero BYTES of LDS (the images with their zero cells); the barrier makes the zeros final before any LDS-DMA piece can land.
template <int BYTES> __device__ __forceinline__ void lp_zero_lds(unsigned char* lds, int tid) {
    for (int i = tid; i < BYTES / 16; i += CW_THREADS) *(cv_u32x4*)(lds + i * 16) = (cv_u32x4){0u, 0u, 0u, 0u};
    CV_BARRIER();
}
// The compiler's wait for the weight loads belongs in front of the tile loop (see az_conv.h): the A fragments are pinned here, the first
// NF_A of them in AGPRs (read by the MFMA in place), the rest in VGPRs.
template <int NF_A, int NF> __device__ __forceinline__ void lp_pin_a(const cv_bf16x8 (&wf)[NF]) {
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        if (f < NF_A) asm volatile("" : : "a"(wf[f]));
        else asm volatile("" : : "v"(wf[f]));
    }
}
// A lane's word of a column tile: LDS byte offset of the (-1, -1) neighbour of its cell in its own lane group's strip (low 16 bits; cell0 =
// the cell of position 0, grp_off = the group's strip offset) | the position it stores (high 16 bits).
__device__ __forceinline__ unsigned lp_lmap(int cell, int cell0, int grp_off, unsigned pos) { return (unsigned)((cell - cell0) * 16 + grp_off) | (pos << 16); }

// ---- LDS-DMA ----------------------------------------------------------------------------------------------------------------------
// One piece: the 64 cells pc of strip c of an image (strips are gblk bytes apart in global memory, lblk in LDS; dst0 = the image's LDS
// address) in one global_load_lds_dwordx4 under the exec mask `mask` (0 = issued, moves nothing: the vm counts do not depend on it);
// lane_src = the lane's byte offset inside the strip (lp_dma_plan).  Inline asm: the compiler neither counts nor reorders it.
__device__ __forceinline__ void lp_dma_piece(const unsigned char* src, unsigned dst0, int c, int pc, int gblk, int lblk, unsigned long long mask, unsigned lane_src) {
    const unsigned long long base = (unsigned long long)(src + (size_t)c * gblk);
    const unsigned dst = dst0 + (unsigned)(c * lblk + pc * 1024);
    asm volatile("s_mov_b64 exec, %0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %3\n\ts_mov_b64 exec, -1"
                 :
                 : "s"(mask), "s"(dst), "v"(lane_src), "s"(base)
                 : "memory");
}
// The lane plan of an image's pieces: src_off(cell) = byte offset of image cell `cell` inside a strip in global memory, or < 0 for a cell
// the DMA never writes (zero cells, cells outside the board) -> per piece the lane's source offset and the exec mask.
template <int NP, class F> __device__ __forceinline__ void lp_dma_plan(unsigned (&dsrc)[NP], unsigned long long (&dmask)[NP], int lane, F src_off) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int o = src_off(64 * i + lane);
        dsrc[i] = (unsigned)(o < 0 ? 0 : o);
        dmask[i] = __builtin_amdgcn_ballot_w64(o >= 0);
    }
}

// ---- epilogue ---------------------------------------------------------------------------------------------------------------------
// y = max(bf16(acc [+ addend]), lo16) of one register quad (4 consecutive couts of a position = an 8-byte slot): the addend's two packed
// dwords are widened half by half, ONE rounding, then the packed-integer ReLU (lo16 = 0: negative floats are negative integers; 0x80008000 =
// no activation).  The riding form: registers + MICRO-OPS of one or two instructions, issued one per MFMA gap by a unit schedule (a 16- or
// 32-cycle MFMA leaves room for about one VALU instruction in its shadow, not for a burst: profiles/r03_block64_ablation.txt).  The adds are
// plain v_add_f32 (cw_add_f32): a v_pk_add_f32 does not fit a gap.  The store that ends a quad is the kernel's (LDS, global, masked or not).
struct LpEpi {
    float ev[4];
    unsigned epa = 0, epb = 0;  // packed halves of the quad in flight
    static constexpr int ops(bool add) { return add ? 9 : 5; }  // micro-ops per quad: [4 adds,] 2 roundings, 2 ReLUs, the store
    // arithmetic micro-op o < ops(ADD) - 1 on the accumulator quad a and the addend words r
    template <bool ADD> __device__ __forceinline__ void op(int o, const lp_f32x4& a, const cv_u32x2& r, unsigned lo16) {
        constexpr int OPS = ops(ADD);
        if (ADD) {
            if (o == 0) ev[0] = cw_add_f32(a[0], cv_bf16_lo(r.x));
            else if (o == 1) ev[1] = cw_add_f32(a[1], cv_bf16_hi(r.x));
            else if (o == 2) ev[2] = cw_add_f32(a[2], cv_bf16_lo(r.y));
            else if (o == 3) ev[3] = cw_add_f32(a[3], cv_bf16_hi(r.y));
            else if (o == 4) epa = cw_pk_bf16(ev[0], ev[1]);
            else if (o == 5) epb = cw_pk_bf16(ev[2], ev[3]);
        } else {
            if (o == 0) epa = cw_pk_bf16(a[0], a[1]);
            else if (o == 1) epb = cw_pk_bf16(a[2], a[3]);
        }
        if (o == OPS - 3) epa = cw_pk_max_i16(epa, lo16);
        else if (o == OPS - 2) epb = cw_pk_max_i16(epb, lo16);
    }
};
// The same arithmetic as ONE block behind a tile's MFMAs (k_conv3x3_t64: no riders, the compiler schedules it and may pack the adds).
template <bool RES> __device__ __forceinline__ cv_u32x2 lp_epi_quad(const lp_f32x4& a, const cv_u32x2& r, unsigned lo16) {
    float v0 = a[0], v1 = a[1], v2 = a[2], v3 = a[3];
    if (RES) {
        v0 += cv_bf16_lo(r.x);
        v1 += cv_bf16_hi(r.x);
        v2 += cv_bf16_lo(r.y);
        v3 += cv_bf16_hi(r.y);
    }
    return (cv_u32x2){cw_pk_max_i16(cw_pk_bf16(v0, v1), lo16), cw_pk_max_i16(cw_pk_bf16(v2, v3), lo16)};
}
#endif  // __HIPCC__
