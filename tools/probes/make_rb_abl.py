"""Ablation builds of the fused split-precision ResNetBlock kernel (az_resblock_sp17.h): copies of the product sources with ONE part of
the kernel removed per build (results are wrong, timings tell what each part costs).  The product header carries no switches: this
script patches copies under /tmp and compiles them to tools/probes/libazsp_abl_RB_<VARIANT>.so, which tools/rb_bench.py times through
AZ_BENCH_LIB.  Variants: FULL (unpatched), NO_DMA (the next tile's LDS-DMA pieces are not issued), NO_VMWAIT (no s_waitcnt vmcnt(0)
in front of a tile's second barrier), NO_BAR (the two barriers of a tile are removed: waves run free), NO_STORE (no y stores, no skip
loads: the compiler drops phase B's epilogue arithmetic as dead code), NO_MWRITE (phase A's epilogue does not write the m image),
NO_FRAG (no B-fragment reads after the first k-steps), NO_EXPOSED (phase A's last unit skips its exposed epilogue).
The epilogue arithmetic, the global stores and the LDS-DMA piece are shared with the other weight-stationary kernels (az_conv_sp.h: SpEpi,
sp_dma_piece); every variant patches this kernel's call site of them, so the sibling kernels of a build stay the product's."""
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-strict-aliasing", "-Wno-unused-value"]


def patch(text, variant):
    def rep(old, new, n=1):
        nonlocal text
        assert text.count(old) == n, (variant, old[:70], text.count(old))
        text = text.replace(old, new)

    if variant == "NO_DMA":
        rep("live ? dmask[h][i % NP] : 0ull", "0ull")
    elif variant == "NO_VMWAIT":
        rep('                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");\n                    CV_BARRIER();', "                    CV_BARRIER();")
    elif variant == "NO_BAR":
        rep('                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");\n                    CV_BARRIER();', "")
        rep("                CV_BARRIER();\n#pragma unroll\n                for (int s = 0; s < R - 1; ++s) load_step(CpInt<1>{}, Ms, NROT, nnj, s, s);",
            "#pragma unroll\n                for (int s = 0; s < R - 1; ++s) load_step(CpInt<1>{}, Ms, NROT, nnj, s, s);")
    elif variant == "NO_STORE":
        rep("else if constexpr (GLOBAL) ep.store(o - 2 * PAIR, out, ooff, store_ok);", "else if constexpr (GLOBAL) ep.store(o - 2 * PAIR, out, ooff, false);")
        rep("                        else rr[set][rj][rp] = *(const cv_u32x2*)(Xs + (lm[ROT][rj].x + skc)", "                        else if (false) rr[set][rj][rp] = *(const cv_u32x2*)(Xs + (lm[ROT][rj].x + skc)")
        rep("                        rrx[rj][rp] = *(const cv_u32x2*)", "                        if (false) rrx[rj][rp] = *(const cv_u32x2*)")
    elif variant == "NO_MWRITE":
        rep("else if (o == 2 * PAIR) *(cv_u32x2*)(Mw + ooff) = (cv_u32x2){ep.hpk[0], ep.hpk[1]};", "else if (o == 2 * PAIR) (void)0;")
        rep("else *(cv_u32x2*)(Mw + MPLANE + ooff) = (cv_u32x2){ep.lpk[0], ep.lpk[1]};", "else (void)0;")
    elif variant == "NO_FRAG":  # load_frag: the per-gap requests inside the units, and (through load_step) the re-starts
        rep("        const int off = sp_frag_off(s, KSUB, G::PITCH, BLK);\n", "        if (it > 0) return;\n        const int off = sp_frag_off(s, KSUB, G::PITCH, BLK);\n")
    elif variant == "NO_EXPOSED":
        rep("                    for (int o = 0; o < CTM; ++o) epi_op(CpInt<0>{}, set, j, lm[ROT][j].y, yprev, o, true);",
            "                    for (int o = 0; o < 0; ++o) epi_op(CpInt<0>{}, set, j, lm[ROT][j].y, yprev, o, true);")
    elif variant != "FULL":
        raise SystemExit("unknown variant " + variant)
    return text


def patched_tree(variant, bd):
    """a copy of the product sources under `bd` with the variant's patch applied; returns the path of the translation unit"""
    shutil.rmtree(bd, ignore_errors=True)
    shutil.copytree(os.path.join(ROOT, "alpha_zero_amd", "csrc"), os.path.join(bd, "alpha_zero_amd", "csrc"))
    shutil.copytree(os.path.join(ROOT, "include"), os.path.join(bd, "include"))
    p = os.path.join(bd, "alpha_zero_amd", "csrc", "az_resblock_sp17.h")
    src = open(p).read()
    if variant == "NO_FRAG":  # `it` must be visible to load_frag: declare the board counter before the lambdas
        src = src.replace("    int it = 0;\n    SpOut yprev =", "    SpOut yprev =").replace("    sp_f16x8 bb[R][2][NJM];", "    int it = 0;\n    sp_f16x8 bb[R][2][NJM];")
    dst = patch(src, variant)
    assert variant == "FULL" or dst != src, variant
    open(p, "w").write(dst)
    return os.path.join(bd, "alpha_zero_amd", "csrc", "azsp_hip.hip")


def build(variant):
    tu = patched_tree(variant, os.path.join("/tmp", "rb_abl_" + variant))
    out = os.path.join(HERE, f"libazsp_abl_RB_{variant}.so")
    subprocess.check_call(["/opt/rocm/bin/hipcc"] + FLAGS + ["-o", out, tu])
    return out


if __name__ == "__main__":
    variants = sys.argv[1:] or ["FULL", "NO_DMA", "NO_VMWAIT", "NO_BAR", "NO_STORE", "NO_MWRITE", "NO_FRAG", "NO_EXPOSED"]
    with ThreadPoolExecutor(8) as ex:
        for o in ex.map(build, variants):
            print("built", o)
