"""Ablation builds of the split-precision tower kernels (az_conv_sp.h, az_conv_sp17.h): copies of the product sources with ONE part of
the kernels removed per build (results are wrong, timings tell what each part costs).  The product headers carry no switches: this
script patches copies under a build directory and compiles them to tools/probes/libazsp_abl_<VARIANT>.so, which tools/split_bench.py
times through AZ_BENCH_LIB.  Variants: FULL (unpatched), HALF_FRAG (B fragments of every second k-step are not read from LDS: the ring
slot keeps its old contents), NO_FRAG (no fragment reads after the first k-steps), NO_DMA (the next tile's LDS-DMA pieces are not
issued), VMCNT0 (NOT an ablation: every counted s_waitcnt vmcnt(N) before a tile barrier replaced by vmcnt(0) -- tools/vmcnt_check.py compares
its outputs bit for bit with the product's), NO_CORNER (9x9: no corner phase), NO_STORE (no output stores and no residual loads; the compiler then drops the whole epilogue arithmetic as dead code).

The pair kernel (az_conv_sp2p.h, k_conv3x3_sp2p) has variants of its own, named SP2P_<X>:
SP2P_NO_STORE (no output stores, unit and corner phase; the epilogue arithmetic stays alive through the range report, so the residual loads stay
too), SP2P_NO_RES (the residual loads of the units and of the corner phase read zeros instead of memory; stores kept), SP2P_NO_DMA (every
LDS-DMA piece is issued with an empty exec mask: no image is fetched), SP2P_VMCNT0 (NOT an ablation: the counted wait in front of an end
barrier becomes vmcnt(0); outputs must stay bit-identical), and the cache-policy variants, which keep every output bit: SP2P_NT_RES (the
residual loads carry nt), SP2P_NT_STORE (the output stores carry nt), SP2P_NT_ALL (both), SP2P_PLAIN_DMA (the global_load_lds_dwordx4 of
dma_piece WITHOUT the nt the product gives it; profiles/sp2p_ablation.txt measured the three nt items on the header that had none), and the
builds around the skewed units, bit-identical as well: SP2P_PLAIN_ORDER (no shared fragments: every unit reads a fragment per live tile in
the plain k-step order, on the product's table), SP2P_EARLY_RES (an item that was measured and left out of the product: the two residual
loads of a corner batch issued in U3 of the batch's last pair instead of in the corner phase) and SP2P_EARLY_RES_PLAIN_ORDER (both patches: the
early corner residual alone).  profiles/sp2p_skew_ab.txt: the product is "shared fragments alone".

The epilogue, the residual load and the LDS-DMA piece of the four weight-stationary kernels are written once, in az_conv_sp.h (SpEpi,
sp_load8, sp_dma_piece).  A variant patches the kernel's CALL SITE of the shared piece wherever that expresses it; the two that change the
store instruction itself (SP2P_NT_STORE, SP2P_NT_ALL) patch SpEpi::store, the one shared place, and so alter the stores of the sibling
kernels in their throw-away build as well (no output bit changes; only time k_conv3x3_sp2p on them).
tools/split_bench.py times several builds in one process (AZ_BENCH_LIBS), tools/split_pmc.py launches them for a counter pass."""
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-strict-aliasing", "-Wno-unused-value"]
SP, SP17, SP2P = "az_conv_sp.h", "az_conv_sp17.h", "az_conv_sp2p.h"


def patch(files, variant):
    """one variant of k_conv3x3_sp / k_conv3x3_sp17: `files` maps header name -> text and is patched in place"""
    def rep(name, old, new, n=1):
        assert files[name].count(old) == n, (variant, name, old[:70], files[name].count(old))
        files[name] = files[name].replace(old, new)

    if variant in ("HALF_FRAG", "NO_FRAG"):
        cond = "(s & 1) == 0" if variant == "HALF_FRAG" else "false"
        for name in (SP, SP17):  # load_frag: the per-gap requests inside the units, and (through load_step) the prologue's
            rep(name, "        const int off = sp_frag_off(s, KSUB, G::PITCH, LBLK);\n", "        if (!(%s)) return;\n        const int off = sp_frag_off(s, KSUB, G::PITCH, LBLK);\n" % cond)
    elif variant == "NO_DMA":
        rep(SP, "live ? dmask[i % NP] : 0ull", "0ull")
        rep(SP17, "live ? dmask[h][i % NP] : 0ull", "0ull")
    elif variant.startswith("SPREAD"):  # the next tile's DMA pieces every STR-th k-step across the units instead of one per k-step in unit 0
        STR = int(variant[6:])
        rep(SP, "                if constexpr (i == 0 && t >= 1 && t - 1 < NPIECE) dma_piece(nsrc, ndst, has_next, t - 1);",
            "                if constexpr (g >= 1 && (g - 1) %% %d == 0 && (g - 1) / %d < NPIECE) dma_piece(nsrc, ndst, has_next, (g - 1) / %d);" % (STR, STR, STR))
        rep(SP, 'if (have_prev) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(VM_YOUNGER) : "memory");', 'if (false) asm volatile("s_nop 0");')
        rep(SP17, "                if constexpr (U == 0 && t >= 1 && t - 1 < NPIECE) dma_piece(nsrc, ndst, nlive, H ^ 1, t - 1);",
            "                if constexpr (g >= 1 && (g - 1) %% %d == 0 && (g - 1) / %d < NPIECE) dma_piece(nsrc, ndst, nlive, H ^ 1, (g - 1) / %d);" % (STR, STR, STR))
        rep(SP17, 'if (H == 0 && !have_prev) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");', 'if (true) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");')
    elif variant == "NO_CORNER":  # 9x9 kernel only: the corner phase (position (8, 0) of the last <= 16 boards) is skipped
        rep(SP, "        if ((it & 15) == 15 || !has_next) {", "        if (false) {")
    elif variant == "VMCNT0":  # every counted s_waitcnt vmcnt(N) in front of a tile barrier becomes vmcnt(0): results must stay bit-identical
        rep(SP, 'if (have_prev) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(VM_YOUNGER) : "memory");', 'if (false) asm volatile("s_nop 0");')
        rep(SP, 'else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // first board', 'asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // first board')
        rep(SP17, 'else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(VM_YOUNGER) : "memory");', 'else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");')
    elif variant == "NO_STORE":
        rep(SP, "else ep.store(o - 2 * PAIR, out, out_off(mj), store_ok);", "else ep.store(o - 2 * PAIR, out, out_off(mj), false);")
        rep(SP17, "else ep.store(o - 2 * PAIR, out, lmap[mj] >> 16, store_ok);", "else ep.store(o - 2 * PAIR, out, lmap[mj] >> 16, false);")
        rep(SP, "                        rr[set][rj][rp] = sp_load8(rbase, rp, out_off(j0 + rj));", "")
        rep(SP17, "                        rr[set][rj][rp] = sp_load8(rbase, rp, lmap[j0 + rj] >> 16);", "")
    else:
        raise SystemExit("unknown variant " + variant)


def patch_sp2p(files, variant):
    """one variant of the pair kernel: az_conv_sp2p.h, and SpEpi::store of az_conv_sp.h for the nt stores"""
    def rep(name, old, new, n=1):
        assert files[name].count(old) == n, (variant, name, old[:70], files[name].count(old))
        files[name] = files[name].replace(old, new)

    ST = "else ep.store(o - 1 - 2 * PAIR, out, out_off(mj), store_ok);"
    ST_HI = "if (store_ok) *(cv_u32x2*)(out.hi + off) = (cv_u32x2){hpk[0], hpk[1]};"  # (SpEpi::store)
    ST_LO = "} else if (store_ok) *(__attribute__((address_space(1))) cv_u32x2*)(out.lo + off) = (cv_u32x2){lpk[0], lpk[1]};"
    CST_HI = "*(cv_u32x2*)(y + co) = (cv_u32x2){sp_pack(h[0], h[1]), sp_pack(h[2], h[3])};"
    CST_LO = "*(cv_u32x2*)(y + co + YPLANE) = (cv_u32x2){sp_pack(l[0], l[1]), sp_pack(l[2], l[3])};"
    LD = "rr[set][rj][rp] = sp_load8(rbase, rp, out_off(j0 + rj));"
    CLD_HI = "rr[0][0][0] = *(const cv_u32x2*)(res + co);"
    CLD_LO = "rr[0][0][1] = *(const cv_u32x2*)(res + co + YPLANE);"
    if variant in ("SP2P_NO_STORE",):
        rep(SP2P, ST, "else ep.store(o - 1 - 2 * PAIR, out, out_off(mj), false);")
        rep(SP2P, CST_HI, "")
        rep(SP2P, CST_LO, "")
    if variant in ("SP2P_NO_RES",):
        rep(SP2P, LD, "rr[set][rj][rp] = (cv_u32x2){0u, 0u};")
        rep(SP2P, CLD_HI, "rr[0][0][0] = (cv_u32x2){0u, 0u};")
        rep(SP2P, CLD_LO, "rr[0][0][1] = (cv_u32x2){0u, 0u};")
    if variant in ("SP2P_NO_DMA",):
        rep(SP2P, "live ? dmask[i % NP] : 0ull", "live && false ? dmask[i % NP] : 0ull")
    if variant in ("SP2P_VMCNT0",):
        rep(SP2P, 'if (pstore) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(VM_YOUNGER) : "memory");', 'if (false) asm volatile("s_nop 0");')
        rep(SP2P, 'else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // first pair', 'asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // first pair')
    if variant in ("SP2P_NT_RES", "SP2P_NT_ALL"):
        rep(SP2P, LD, "rr[set][rj][rp] = rp == 0 ? __builtin_nontemporal_load((const cv_u32x2*)(rbase.hi + out_off(j0 + rj)))"
            " : __builtin_nontemporal_load((const __attribute__((address_space(1))) cv_u32x2*)(rbase.lo + out_off(j0 + rj)));")
        rep(SP2P, CLD_HI, "rr[0][0][0] = __builtin_nontemporal_load((const cv_u32x2*)(res + co));")
        rep(SP2P, CLD_LO, "rr[0][0][1] = __builtin_nontemporal_load((const cv_u32x2*)(res + co + YPLANE));")
    if variant in ("SP2P_PLAIN_DMA",):
        rep(SP2P, "sp_dma_piece<true>(", "sp_dma_piece<false>(")
    if variant in ("SP2P_NT_STORE", "SP2P_NT_ALL"):
        rep(SP, ST_HI, "if (store_ok) __builtin_nontemporal_store((cv_u32x2){hpk[0], hpk[1]}, (cv_u32x2*)(out.hi + off));")
        rep(SP, ST_LO, "} else if (store_ok) __builtin_nontemporal_store((cv_u32x2){lpk[0], lpk[1]}, (__attribute__((address_space(1))) cv_u32x2*)(out.lo + off));")
        rep(SP2P, CST_HI, "__builtin_nontemporal_store((cv_u32x2){sp_pack(h[0], h[1]), sp_pack(h[2], h[3])}, (cv_u32x2*)(y + co));")
        rep(SP2P, CST_LO, "__builtin_nontemporal_store((cv_u32x2){sp_pack(l[0], l[1]), sp_pack(l[2], l[3])}, (cv_u32x2*)(y + co + YPLANE));")
    if variant in ("SP2P_PLAIN_ORDER", "SP2P_EARLY_RES_PLAIN_ORDER"):
        rep(SP2P, "s.shared = sp2p_row_shifts(sp2p_map_table, u);", "s.shared = false;")
        rep(SP2P, "static_assert(Sp2pU<0>::S.ns == 30 && Sp2pU<3>::S.ns == 24 &&", "static_assert(Sp2pU<0>::S.ns == 18 && Sp2pU<3>::S.ns == 18 &&")
        rep(SP2P, "static_assert(Sp2pU<0>::S.reads() == 60 && Sp2pU<1>::S.reads() == 60 && Sp2pU<2>::S.reads() == 84 && Sp2pU<3>::S.reads() == 48,",
            "static_assert(Sp2pU<0>::S.reads() == 108 && Sp2pU<1>::S.reads() == 60 && Sp2pU<2>::S.reads() == 84 && Sp2pU<3>::S.reads() == 72,")
        rep(SP2P, "static_assert(Sp2pU<0>::S.nfrag(0) == 1,", "static_assert(Sp2pU<0>::S.nfrag(0) == 3,")
        rep(SP2P, "        frag_req(CpInt<0>{}, CpInt<0>{}, CpInt<1>{});\n", "".join("        frag_req(CpInt<0>{}, CpInt<0>{}, CpInt<%d>{});\n" % q for q in range(1, 6)))
    if variant in ("SP2P_EARLY_RES", "SP2P_EARLY_RES_PLAIN_ORDER"):
        # the loads move from the corner phase into slots 2 nj, 2 nj + 1 of U3 (behind U3's own residual loads, in front of its first LDS-DMA piece: the
        # counted wait of U3's end barrier covers them), on the last pair of a corner batch, into set 1's third rr entry, which a two-tile unit leaves free
        rep(SP2P, "        const bool have_prev = it > 0;\n", """        const bool have_prev = it > 0;
        const bool corner_next = cb + 2 == SP2P_NB || !has_next;
        auto corner_off = [&](int n_ok) __attribute__((always_inline)) {
            const int it0 = it - (n_ok / 2 - 1), nb = l15 < n_ok ? l15 : 0;
            const size_t board = 2 * ((size_t)slot + (size_t)(it0 + (nb >> 1)) * nslot) + (nb & 1);
            return board * YTILE + (size_t)(cg * 8 + wa * 4 + wb * 2 + (kg >> 1)) * GBLK + G::CORNER * 16 + (kg & 1) * 8;
        };
""")
        rep(SP2P, "                __builtin_amdgcn_sched_barrier(0);\n                if constexpr (K::DMA &&", """                if constexpr (RES && u == 3 && sl >= 2 * nj && sl < 2 * nj + 2) {
                    static_assert(2 * nj + 2 <= K::PFIRST && nj < NJ0, "older than the pieces; a free rr entry");
                    if (corner_next) rr[1][NJ0 - 1][sl - 2 * nj] = *(const cv_u32x2*)(res + corner_off(cb + 2) + (sl - 2 * nj) * YPLANE);
                }
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (K::DMA &&""")
        rep(SP2P, CLD_HI, "")
        rep(SP2P, CLD_LO, "")
        rep(SP2P, "const cv_u32x2 rh = rr[0][0][0], rl = rr[0][0][1];", "const cv_u32x2 rh = rr[1][NJ0 - 1][0], rl = rr[1][NJ0 - 1][1];")


SP2P_VARIANTS = ("SP2P_NO_STORE", "SP2P_NO_RES", "SP2P_NO_DMA", "SP2P_VMCNT0", "SP2P_NT_RES", "SP2P_NT_STORE", "SP2P_NT_ALL", "SP2P_PLAIN_DMA", "SP2P_PLAIN_ORDER", "SP2P_EARLY_RES", "SP2P_EARLY_RES_PLAIN_ORDER")


def patched_tree(variant, bd):
    """a copy of the product sources under `bd` with the variant's patch applied; returns the path of the translation unit"""
    shutil.rmtree(bd, ignore_errors=True)
    shutil.copytree(os.path.join(ROOT, "alpha_zero_amd", "csrc"), os.path.join(bd, "alpha_zero_amd", "csrc"))
    shutil.copytree(os.path.join(ROOT, "include"), os.path.join(bd, "include"))
    if variant != "FULL":
        src = {name: open(os.path.join(bd, "alpha_zero_amd", "csrc", name)).read() for name in (SP, SP17, SP2P)}
        files = dict(src)
        if variant.startswith("SP2P_"):
            assert variant in SP2P_VARIANTS, variant
            patch_sp2p(files, variant)
        else:
            patch(files, variant)
        assert files != src, variant
        for name, text in files.items():
            open(os.path.join(bd, "alpha_zero_amd", "csrc", name), "w").write(text)
    return os.path.join(bd, "alpha_zero_amd", "csrc", "azsp_hip.hip")


def build(variant):
    tu = patched_tree(variant, os.path.join("/tmp", "sp_abl_" + variant))
    out = os.path.join(HERE, f"libazsp_abl_{variant}.so")
    subprocess.check_call(["/opt/rocm/bin/hipcc"] + FLAGS + ["-o", out, tu])
    return out


if __name__ == "__main__":
    variants = sys.argv[1:] or ["HALF_FRAG", "NO_FRAG", "NO_DMA", "NO_STORE"]
    with ThreadPoolExecutor(4) as ex:
        for o in ex.map(build, variants):
            print("built", o)
