"""k_conv3x3_sp2p without a GPU: its column-tile table is the generated one, and its fragment reads sit one per MFMA gap (the disassembly
property of tests/test_kernel_schedule.py, same thresholds)."""
import os
import re
import subprocess
import sys
from collections import Counter

import pytest

import test_kernel_schedule as ks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pair_tile_map_in_the_header_is_the_generated_one():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_sp_map_pair.py")], capture_output=True, text=True, check=True).stdout
    gen = [int(v) for v in re.findall(r"\d+", out.split("\n", 1)[1])]
    hdr = open(os.path.join(ROOT, "alpha_zero_amd", "csrc", "az_conv_sp2p.h")).read()
    body = hdr[hdr.index("constexpr Sp2pMap sp2p_map_table = {{") :]
    tab = [int(v) for v in re.findall(r"\d+", body[: body.index("}};")].split("\n", 2)[2])]
    assert len(gen) == 160 and gen == tab
    assert sorted(gen) == [b * 81 + p for b in range(2) for p in range(81) if p != 72]  # both boards, every position but the corner (8, 0), once
    assert out.split("\n", 1)[0] in hdr  # (the comment line names seed and trial)


@pytest.mark.skipif(not os.path.exists(ks.OBJDUMP), reason="llvm-objdump of the ROCm image")
def test_pair_kernel_fragment_reads_sit_in_mfma_gaps_of_their_own():
    kernels = ks._reads_per_mfma_gap("k_conv3x3_sp2pI")
    assert len(kernels) == 2, list(kernels)
    for name, reads in kernels.items():
        hist = Counter(reads)
        bursts = sum(n for k, n in hist.items() if k > 2)
        assert len(reads) > 250 and bursts <= 0, (name, sorted(hist.items()))
        assert hist[1] >= 0.25 * len(reads), (name, sorted(hist.items()))
