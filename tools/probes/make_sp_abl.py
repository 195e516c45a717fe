"""Ablation builds of the split-precision tower kernels (az_conv_sp.h, az_conv_sp17.h): copies of the product sources with ONE part of
the kernels removed per build (results are wrong, timings tell what each part costs).  The product headers carry no switches: this
script patches copies under a build directory and compiles them to tools/probes/libazsp_abl_<VARIANT>.so, which tools/split_bench.py
times through AZ_BENCH_LIB.  Variants: FULL (unpatched), HALF_FRAG (B fragments of every second k-step are not read from LDS: the ring
slot keeps its old contents), NO_FRAG (no fragment reads after the first k-steps), NO_DMA (the next tile's LDS-DMA pieces are not
issued), VMCNT0 (NOT an ablation: every counted s_waitcnt vmcnt(N) before a tile barrier replaced by vmcnt(0) -- tools/vmcnt_check.py compares
its outputs bit for bit with the product's), NO_CORNER (9x9: no corner phase), NO_STORE (no output stores and no residual loads; the compiler then drops the whole epilogue arithmetic as dead code).

The pair kernel (az_conv_sp2p.h, k_conv3x3_sp2p) has variants of its own, named SP2P_<X>; they patch a copy of az_conv_sp2p.h only:
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
tools/split_bench.py times several builds in one process (AZ_BENCH_LIBS), tools/split_pmc.py launches them for a counter pass."""
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-strict-aliasing", "-Wno-unused-value"]


def patch(text, variant, name):
    def rep(old, new, count=1):
        nonlocal text
        assert text.count(old) >= 1, (name, old[:60])
        text = text.replace(old, new) if count == 0 else text.replace(old, new, count)

    if variant in ("HALF_FRAG", "NO_FRAG"):
        cond = "(s & 1) == 0" if variant == "HALF_FRAG" else "false"
        # (every occurrence: load_step of the prologue AND load_frag, the per-gap requests inside the units since the end of round 6)
        rep("        const int tap = s / KSUB;\n        const int off =", "        if (!(%s)) return;\n        const int tap = s / KSUB;\n        const int off =" % cond, 0)
    elif variant == "NO_DMA":
        rep("        const unsigned long long mask = live ? dmask", "        live = false;\n        const unsigned long long mask = live ? dmask")
    elif variant.startswith("SPREAD"):  # the next tile's DMA pieces every STR-th k-step across the units instead of one per k-step in unit 0
        STR = int(variant[6:])
        if name == "az_conv_sp.h":
            rep("                if constexpr (i == 0 && t >= 1 && t - 1 < NPIECE) dma_piece(nsrc, ndst, has_next, t - 1);",
                "                if constexpr (g >= 1 && (g - 1) %% %d == 0 && (g - 1) / %d < NPIECE) dma_piece(nsrc, ndst, has_next, (g - 1) / %d);" % (STR, STR, STR))
            rep('if (have_prev) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(VM_YOUNGER) : "memory");', 'if (false) asm volatile("s_nop 0");')
        else:
            rep("                if constexpr (U == 0 && t >= 1 && t - 1 < NPIECE) dma_piece(nsrc, ndst, nlive, H ^ 1, t - 1);",
                "                if constexpr (g >= 1 && (g - 1) %% %d == 0 && (g - 1) / %d < NPIECE) dma_piece(nsrc, ndst, nlive, H ^ 1, (g - 1) / %d);" % (STR, STR, STR))
            rep('if (H == 0 && !have_prev) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");', 'if (true) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");')
    elif variant == "NO_CORNER":  # 9x9 kernel only: the corner phase (position (8, 0) of the last <= 16 boards) is skipped
        if name == "az_conv_sp.h":
            rep("        if ((it & 15) == 15 || !has_next) {", "        if (false) {")
    elif variant == "VMCNT0":  # every counted s_waitcnt vmcnt(N) in front of a tile barrier becomes vmcnt(0): results must stay bit-identical
        if name == "az_conv_sp.h":
            rep('if (have_prev) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(VM_YOUNGER) : "memory");', 'if (false) asm volatile("s_nop 0");')
            rep('else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // first board', 'asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // first board')
        else:
            rep('else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(VM_YOUNGER) : "memory");', 'else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");')
    elif variant == "NO_STORE":
        rep("if (store_ok) *(cv_u32x2*)", "if (false) *(cv_u32x2*)", 0)
        rep("} else if (store_ok) *(__attribute__((address_space(1))) cv_u32x2*)", "} else if (false) *(__attribute__((address_space(1))) cv_u32x2*)", 0)
        rep("                        if constexpr (rp == 0) rr[set][rj][rp] = *(const cv_u32x2*)", "                        if constexpr (false) rr[set][rj][rp] = *(const cv_u32x2*)")
        rep("                        else rr[set][rj][rp] = *(const __attribute__((address_space(1))) cv_u32x2*)",
            "                        else if constexpr (false) rr[set][rj][rp] = *(const __attribute__((address_space(1))) cv_u32x2*)")
    return text


def patch_sp2p(text, variant):
    """one variant of the pair kernel: a patched copy of az_conv_sp2p.h"""
    def rep(old, new, n):
        nonlocal text
        assert text.count(old) == n, (variant, old[:70], text.count(old))
        text = text.replace(old, new)

    ST_HI = "if (store_ok) *(cv_u32x2*)(out + gq) = (cv_u32x2){hpk[0], hpk[1]};"
    ST_LO = "} else if (store_ok) *(__attribute__((address_space(1))) cv_u32x2*)(out_lo + gq) = (cv_u32x2){lpk[0], lpk[1]};"
    CST_HI = "*(cv_u32x2*)(y + co) = (cv_u32x2){sp_pack(h[0], h[1]), sp_pack(h[2], h[3])};"
    CST_LO = "*(cv_u32x2*)(y + co + YPLANE) = (cv_u32x2){sp_pack(l[0], l[1]), sp_pack(l[2], l[3])};"
    LD_HI = "rr[set][rj][rp] = *(const cv_u32x2*)(rbase + out_off(j0 + rj));"
    LD_LO = "rr[set][rj][rp] = *(const __attribute__((address_space(1))) cv_u32x2*)(rbase_lo + out_off(j0 + rj));"
    CLD_HI = "rr[0][0][0] = *(const cv_u32x2*)(res + co);"
    CLD_LO = "rr[0][0][1] = *(const cv_u32x2*)(res + co + YPLANE);"
    DMA = "global_load_lds_dwordx4 %2, %3 nt\\n"
    if variant in ("SP2P_NO_STORE",):
        rep(ST_HI, "if (false) {}", 1)
        rep(ST_LO, "} else if (false) {}", 1)
        rep(CST_HI, "", 1)
        rep(CST_LO, "", 1)
    if variant in ("SP2P_NO_RES",):
        for old in (LD_HI, LD_LO):
            rep(old, "rr[set][rj][rp] = (cv_u32x2){0u, 0u};", 1)
        rep(CLD_HI, "rr[0][0][0] = (cv_u32x2){0u, 0u};", 1)
        rep(CLD_LO, "rr[0][0][1] = (cv_u32x2){0u, 0u};", 1)
    if variant in ("SP2P_NO_DMA",):
        rep("const unsigned long long mask = live ? dmask[pc] : 0ull;", "const unsigned long long mask = live && false ? dmask[pc] : 0ull;", 1)
    if variant in ("SP2P_VMCNT0",):
        rep('if (pstore) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(VM_YOUNGER) : "memory");', 'if (false) asm volatile("s_nop 0");', 1)
        rep('else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // first pair', 'asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // first pair', 1)
    if variant in ("SP2P_NT_RES", "SP2P_NT_ALL"):
        rep(LD_HI, "rr[set][rj][rp] = __builtin_nontemporal_load((const cv_u32x2*)(rbase + out_off(j0 + rj)));", 1)
        rep(LD_LO, "rr[set][rj][rp] = __builtin_nontemporal_load((const __attribute__((address_space(1))) cv_u32x2*)(rbase_lo + out_off(j0 + rj)));", 1)
        rep(CLD_HI, "rr[0][0][0] = __builtin_nontemporal_load((const cv_u32x2*)(res + co));", 1)
        rep(CLD_LO, "rr[0][0][1] = __builtin_nontemporal_load((const cv_u32x2*)(res + co + YPLANE));", 1)
    if variant in ("SP2P_PLAIN_DMA",):
        rep(DMA, "global_load_lds_dwordx4 %2, %3\\n", 1)
    if variant in ("SP2P_NT_STORE", "SP2P_NT_ALL"):
        rep(ST_HI, "if (store_ok) __builtin_nontemporal_store((cv_u32x2){hpk[0], hpk[1]}, (cv_u32x2*)(out + gq));", 1)
        rep(ST_LO, "} else if (store_ok) __builtin_nontemporal_store((cv_u32x2){lpk[0], lpk[1]}, (__attribute__((address_space(1))) cv_u32x2*)(out_lo + gq));", 1)
        rep(CST_HI, "__builtin_nontemporal_store((cv_u32x2){sp_pack(h[0], h[1]), sp_pack(h[2], h[3])}, (cv_u32x2*)(y + co));", 1)
        rep(CST_LO, "__builtin_nontemporal_store((cv_u32x2){sp_pack(l[0], l[1]), sp_pack(l[2], l[3])}, (cv_u32x2*)(y + co + YPLANE));", 1)
    if variant in ("SP2P_PLAIN_ORDER", "SP2P_EARLY_RES_PLAIN_ORDER"):
        rep("s.shared = sp2p_row_shifts(sp2p_map_table, u);", "s.shared = false;", 1)
        rep("static_assert(Sp2pU<0>::S.ns == 30 && Sp2pU<3>::S.ns == 24 &&", "static_assert(Sp2pU<0>::S.ns == 18 && Sp2pU<3>::S.ns == 18 &&", 1)
        rep("static_assert(Sp2pU<0>::S.reads() == 60 && Sp2pU<1>::S.reads() == 60 && Sp2pU<2>::S.reads() == 84 && Sp2pU<3>::S.reads() == 48,",
            "static_assert(Sp2pU<0>::S.reads() == 108 && Sp2pU<1>::S.reads() == 60 && Sp2pU<2>::S.reads() == 84 && Sp2pU<3>::S.reads() == 72,", 1)
        rep("static_assert(Sp2pU<0>::S.nfrag(0) == 1,", "static_assert(Sp2pU<0>::S.nfrag(0) == 3,", 1)
        rep("        frag_req(CpInt<0>{}, CpInt<0>{}, CpInt<1>{});\n", "".join("        frag_req(CpInt<0>{}, CpInt<0>{}, CpInt<%d>{});\n" % q for q in range(1, 6)), 1)
    if variant in ("SP2P_EARLY_RES", "SP2P_EARLY_RES_PLAIN_ORDER"):
        # the loads move from the corner phase into slots 2 nj, 2 nj + 1 of U3 (behind U3's own residual loads, in front of its first LDS-DMA piece: the
        # counted wait of U3's end barrier covers them), on the last pair of a corner batch, into set 1's third rr entry, which a two-tile unit leaves free
        rep("        const bool have_prev = it > 0;\n", """        const bool have_prev = it > 0;
        const bool corner_next = cb + 2 == SP2P_NB || !has_next;
        auto corner_off = [&](int n_ok) __attribute__((always_inline)) {
            const int it0 = it - (n_ok / 2 - 1), nb = l15 < n_ok ? l15 : 0;
            const size_t board = 2 * ((size_t)slot + (size_t)(it0 + (nb >> 1)) * nslot) + (nb & 1);
            return board * YTILE + (size_t)(cg * 8 + wa * 4 + wb * 2 + (kg >> 1)) * GBLK + G::CORNER * 16 + (kg & 1) * 8;
        };
""", 1)
        rep("                __builtin_amdgcn_sched_barrier(0);\n                if constexpr (K::DMA &&", """                if constexpr (RES && u == 3 && sl >= 2 * nj && sl < 2 * nj + 2) {
                    static_assert(2 * nj + 2 <= K::PFIRST && nj < NJ0, "older than the pieces; a free rr entry");
                    if (corner_next) rr[1][NJ0 - 1][sl - 2 * nj] = *(const cv_u32x2*)(res + corner_off(cb + 2) + (sl - 2 * nj) * YPLANE);
                }
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (K::DMA &&""", 1)
        rep(CLD_HI, "", 1)
        rep(CLD_LO, "", 1)
        rep("const cv_u32x2 rh = rr[0][0][0], rl = rr[0][0][1];", "const cv_u32x2 rh = rr[1][NJ0 - 1][0], rl = rr[1][NJ0 - 1][1];", 1)
    return text


SP2P_VARIANTS = ("SP2P_NO_STORE", "SP2P_NO_RES", "SP2P_NO_DMA", "SP2P_VMCNT0", "SP2P_NT_RES", "SP2P_NT_STORE", "SP2P_NT_ALL", "SP2P_PLAIN_DMA", "SP2P_PLAIN_ORDER", "SP2P_EARLY_RES", "SP2P_EARLY_RES_PLAIN_ORDER")


def build(variant):
    bd = os.path.join("/tmp", "sp_abl_" + variant)
    shutil.rmtree(bd, ignore_errors=True)
    shutil.copytree(os.path.join(ROOT, "alpha_zero_amd", "csrc"), os.path.join(bd, "alpha_zero_amd", "csrc"))
    shutil.copytree(os.path.join(ROOT, "include"), os.path.join(bd, "include"))
    if variant.startswith("SP2P_"):
        assert variant in SP2P_VARIANTS, variant
        p = os.path.join(bd, "alpha_zero_amd", "csrc", "az_conv_sp2p.h")
        src = open(p).read()
        dst = patch_sp2p(src, variant)
        assert dst != src, variant
        open(p, "w").write(dst)
    elif variant != "FULL":
        for name in ("az_conv_sp.h", "az_conv_sp17.h"):
            p = os.path.join(bd, "alpha_zero_amd", "csrc", name)
            src = open(p).read()
            open(p, "w").write(patch(src, variant, name))
    out = os.path.join(HERE, f"libazsp_abl_{variant}.so")
    subprocess.check_call(["/opt/rocm/bin/hipcc"] + FLAGS + ["-o", out, os.path.join(bd, "alpha_zero_amd", "csrc", "azsp_hip.hip")])
    return out


if __name__ == "__main__":
    variants = sys.argv[1:] or ["HALF_FRAG", "NO_FRAG", "NO_DMA", "NO_STORE"]
    with ThreadPoolExecutor(4) as ex:
        for o in ex.map(build, variants):
            print("built", o)
