"""Same-box, same-process A/B of the fp32-class tower kernels of two builds of the library: the one in the tree against another build
(default tools/probes/libazsp_prev.so), timed alternately on the same post-ReLU-like activations, with a bitwise comparison of the outputs
(each build into a buffer of its own; the timed launches of every build then write ONE buffer).
Cases: the 9x9 x 128 convolution (k_conv3x3_sp2p, plain and with a residual), the 9x9 x 64 and 17x17 x 64 convolutions (k_conv3x3_sp<.., 8, 1>,
k_conv3x3_sp17<.., 8>, plain and with a residual), the fused 17x17 x 64 and 9x9 x 64 blocks (k_resblock_sp<Sb17 | Sb9>), the three tailored stems
(9x9 -> 128, 9x9 -> 64, 13x13 pad 3 -> 17x17 x 64: k_conv3x3_sp / k_conv3x3_sp17 with 4 input chunks) through azsp_stem_split (random fp32 planes)
and azsp_stem_split_exact (0 / 1 planes); and the lower-precision (bf16) kernels through the tiled ABI: azsp_conv3x3_tiled at 9x9 x 64 and
17x17 x 64 (k_conv3x3_t64) and at 19x19 x 256 (k_conv3x3_op19q; k_conv3x3_hb19 twice in a process started with AZSP_CONV19_TWO_LAUNCH=1), plain
and with a residual, azsp_resblock_tiled at both 64-filter geometries (k_resblock64), azsp_stem_tiled at 9x9 -> 64, 13x13 pad 3 -> 64
(k_conv3x3_t64 with 4 input chunks) and 19x19 -> 256 (k_conv3x3_hb19 with 4).  PREV_AB_CASES=<substring>[,<substring>...] selects cases.  other_lib may be a comma-separated list: with a second COPY of the other build (another file) the same run also gives the A/A
spread of every case -- the margin below which a tree / other ratio says nothing.
usage: python tools/split_prev_ab.py [other_lib[,other_lib2...]] [rounds]"""
import ctypes
import functools
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from alpha_zero_amd import _abi, _lib
from alpha_zero_amd.core.network import split_weights_f16

other = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tools", "probes", "libazsp_prev.so")
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
libs = {"tree": _lib.load()}
for i, path in enumerate(other.split(",")):
    libs["other" if i == 0 else f"other{i + 1}"] = _abi.Binding(ctypes.CDLL(path), "A/B build")
st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
B = 32768


@functools.lru_cache(maxsize=1)  # (a shape's plain and residual case follow each other and share their tensors)
def make(S, C, seed):
    g = torch.Generator().manual_seed(seed)

    def act():
        t = torch.randn(B, C, S, S, generator=g)
        return torch.where(torch.rand(B, C, S, S, generator=g) < 0.5, torch.zeros(()), t.abs()).cuda().contiguous(memory_format=torch.channels_last)

    d = libs["tree"].dll
    n = d.azsp_split_bytes(B, S, C) // 2
    xs, rs = (torch.zeros(n, dtype=torch.float16, device="cuda") for _ in range(2))
    for src, dst in ((act(), xs), (act(), rs)):
        assert d.azsp_split_layout(src.data_ptr(), dst.data_ptr(), B, S, C, 1, None, st) == 0
    ws = [split_weights_f16(torch.randn(C, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5).cuda() for _ in range(2)]
    bs = [(torch.randn(C, generator=g) * 0.1).cuda() for _ in range(2)]
    ys = {k: torch.zeros(n, dtype=torch.float16, device="cuda") for k in libs}
    torch.cuda.synchronize()
    return xs, rs, ws, bs, ys


def case_conv(S, C, residual):
    xs, rs, ws, bs, ys = make(S, C, 1)

    def run(k, reps, o=None):
        for _ in range(reps):
            assert libs[k].dll.azsp_conv3x3_split(xs.data_ptr(), ws[0].data_ptr(), bs[0].data_ptr(), rs.data_ptr() if residual else None, ys[o or k].data_ptr(), B, S, C, 1, None, st) == 0

    return run, ys, 2.0 * B * S * S * C * C * 9 * 3


def case_block(S, C):
    xs, rs, ws, bs, ys = make(S, C, 2)

    def run(k, reps, o=None):
        for _ in range(reps):
            assert libs[k].dll.azsp_resblock_split(xs.data_ptr(), ws[0].data_ptr(), bs[0].data_ptr(), ws[1].data_ptr(), bs[1].data_ptr(), ys[o or k].data_ptr(), B, S, C, None, st) == 0

    return run, ys, 2 * 2.0 * B * S * S * C * C * 9 * 3


def case_stem(n, pad, C, exact):
    """a tailored stem: n x n boards of 17 planes (exact: 0 / 1 planes through azsp_stem_split_exact, else random fp32 planes) -> C filters"""
    S = n + 2 * (pad - 1)
    d = libs["tree"].dll
    g = torch.Generator().manual_seed(4)
    x = ((torch.rand(B, 17, n, n, generator=g) > 0.6).float() if exact else torch.randn(B, 17, n, n, generator=g)).cuda()
    feat = torch.zeros(d.azsp_split_bytes(B, n, 32) // 2, dtype=torch.float16, device="cuda")
    assert d.azsp_split_features(x.data_ptr(), feat.data_ptr(), B, n, 17, None, st) == 0
    w32 = torch.zeros(C, 32, 3, 3)
    w32[:, :17] = torch.randn(C, 17, 3, 3, generator=g) * 0.1
    w, bias = split_weights_f16(w32).cuda(), (torch.randn(C, generator=g) * 0.1).cuda()
    ys = {k: torch.zeros(d.azsp_split_bytes(B, S, C) // 2, dtype=torch.float16, device="cuda") for k in libs}
    torch.cuda.synchronize()

    def run(k, reps, o=None):
        entry = libs[k].dll.azsp_stem_split_exact if exact else libs[k].dll.azsp_stem_split
        for _ in range(reps):
            assert entry(feat.data_ptr(), w.data_ptr(), bias.data_ptr(), ys[o or k].data_ptr(), B, n, C, pad, 1, None, st) == 0

    return run, ys, 2.0 * B * S * S * 32 * C * 9 * (2 if exact else 3)


TILED_BOARDS = {9: 12288, 17: 4096, 19: 4096}  # 4096 tiles (9x9: three boards per tile) = 16 per workgroup


@functools.lru_cache(maxsize=1)
def make_tiled(S, C, seed):
    """bf16 activations x, r in the tiled layout, two packed weight banks, two biases, an output per build"""
    boards, d, g = TILED_BOARDS[S], libs["tree"].dll, torch.Generator().manual_seed(seed)
    n = d.azsp_tiled_bytes(boards, S, C) // 2
    xt, rt = (torch.zeros(n, dtype=torch.bfloat16, device="cuda") for _ in range(2))
    for dst in (xt, rt):
        t = torch.randn(boards, C, S, S, generator=g)
        t = torch.where(torch.rand(boards, C, S, S, generator=g) < 0.5, torch.zeros(()), t.abs()).to(torch.bfloat16).cuda().contiguous(memory_format=torch.channels_last)
        assert d.azsp_tile_layout(t.data_ptr(), dst.data_ptr(), boards, S, C, 1, None) == 0
        del t
    ws = [(torch.randn(C, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5).to(torch.bfloat16).cuda().permute(2, 3, 0, 1).reshape(9, C, C).contiguous() for _ in range(2)]
    bs = [(torch.randn(C, generator=g) * 0.1).cuda() for _ in range(2)]
    ys = {k: torch.zeros(n, dtype=torch.bfloat16, device="cuda") for k in libs}
    torch.cuda.synchronize()
    return boards, xt, rt, ws, bs, ys


def case_conv_tiled(S, C, residual):
    """a bf16 tower convolution through azsp_conv3x3_tiled (19x19 x 256: BASELINE C5's dominant kernel)"""
    boards, xt, rt, ws, bs, ys = make_tiled(S, C, 3)

    def run(k, reps, o=None):
        for _ in range(reps):
            assert libs[k].dll.azsp_conv3x3_tiled(xt.data_ptr(), ws[0].data_ptr(), bs[0].data_ptr(), rt.data_ptr() if residual else None, ys[o or k].data_ptr(), boards, S, C, 1, st) == 0

    return run, ys, 2.0 * boards * S * S * C * C * 9


def case_block_tiled(S, C):
    boards, xt, rt, ws, bs, ys = make_tiled(S, C, 5)

    def run(k, reps, o=None):
        for _ in range(reps):
            assert libs[k].dll.azsp_resblock_tiled(xt.data_ptr(), ws[0].data_ptr(), bs[0].data_ptr(), ws[1].data_ptr(), bs[1].data_ptr(), ys[o or k].data_ptr(), boards, S, C, st) == 0

    return run, ys, 2 * 2.0 * boards * S * S * C * C * 9


def case_stem_tiled(n, pad, C):
    """a bf16 stem: n x n boards of 17 planes in 32 tiled channels -> C filters on planes of n + 2 (pad - 1)"""
    S, d, g = n + 2 * (pad - 1), libs["tree"].dll, torch.Generator().manual_seed(6)
    boards = TILED_BOARDS[S]
    x = torch.zeros(boards, 32, n, n)
    x[:, :17] = (torch.rand(boards, 17, n, n, generator=g) > 0.6).float()
    feat = torch.zeros(d.azsp_tiled_bytes(boards, n, 32) // 2, dtype=torch.bfloat16, device="cuda")
    xc = x.to(torch.bfloat16).cuda().contiguous(memory_format=torch.channels_last)
    assert d.azsp_tile_layout(xc.data_ptr(), feat.data_ptr(), boards, n, 32, 1, None) == 0
    w32 = torch.zeros(C, 32, 3, 3)
    w32[:, :17] = torch.randn(C, 17, 3, 3, generator=g) * 0.1
    w, bias = w32.to(torch.bfloat16).cuda().permute(2, 3, 0, 1).reshape(9, C, 32).contiguous(), (torch.randn(C, generator=g) * 0.1).cuda()
    ys = {k: torch.zeros(d.azsp_tiled_bytes(boards, S, C) // 2, dtype=torch.bfloat16, device="cuda") for k in libs}
    torch.cuda.synchronize()

    def run(k, reps, o=None):
        for _ in range(reps):
            assert libs[k].dll.azsp_stem_tiled(feat.data_ptr(), w.data_ptr(), bias.data_ptr(), ys[o or k].data_ptr(), boards, n, C, pad, 1, st) == 0

    return run, ys, 2.0 * boards * S * S * 32 * C * 9


CASES = (("conv 9x9 x 128 plain", lambda: case_conv(9, 128, False)), ("conv 9x9 x 128 residual", lambda: case_conv(9, 128, True)),
         ("conv 9x9 x 64 plain", lambda: case_conv(9, 64, False)), ("conv 9x9 x 64 residual", lambda: case_conv(9, 64, True)),
         ("conv 17x17 x 64 plain", lambda: case_conv(17, 64, False)), ("conv 17x17 x 64 residual", lambda: case_conv(17, 64, True)),
         ("block 17x17 x 64", lambda: case_block(17, 64)), ("block 9x9 x 64", lambda: case_block(9, 64)),
         *((f"stem {n}x{n} pad {pad} -> {C}{' exact' if exact else ''}", lambda n=n, pad=pad, C=C, exact=exact: case_stem(n, pad, C, exact))
           for n, pad, C in ((9, 1, 128), (9, 1, 64), (13, 3, 64)) for exact in (False, True)),
         *((f"conv {S}x{S} x {C} bf16 {'residual' if res else 'plain'}", lambda S=S, C=C, res=res: case_conv_tiled(S, C, res))
           for S, C in ((9, 64), (17, 64), (19, 256)) for res in (False, True)),
         ("block 9x9 x 64 bf16", lambda: case_block_tiled(9, 64)), ("block 17x17 x 64 bf16", lambda: case_block_tiled(17, 64)),
         *((f"stem {n}x{n} pad {pad} -> {C} bf16", lambda n=n, pad=pad, C=C: case_stem_tiled(n, pad, C)) for n, pad, C in ((9, 1, 64), (13, 3, 64), (19, 1, 256))))
ONLY = os.environ.get("PREV_AB_CASES", "").split(",")
for name, mk in [c for c in CASES if any(o in c[0] for o in ONLY)]:
    run, ys, flops = mk()
    for k in libs:
        run(k, 3)
    torch.cuda.synchronize()
    print(f"{name}: bit-identical outputs: {all(torch.equal(ys['tree'], ys[k]) for k in libs)}", flush=True)
    tot = {k: 0.0 for k in libs}
    for rnd in range(ROUNDS):
        for k in (list(libs) if rnd % 2 == 0 else list(libs)[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(k, 30, "tree")  # (every build writes the SAME buffer: where an output lies decides a write-bound kernel's time by several per cent)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / 30
            tot[k] += ms if rnd > 0 else 0.0  # (round 0 warms the clocks up)
            print(f"  round {rnd} {k:6s} {ms:7.4f} ms  frac {flops / ms / 1e9 / 2500:.4f}", flush=True)
    print("  mean of rounds 1.. : " + ", ".join(f"{k} {v / (ROUNDS - 1):.4f} ms" for k, v in tot.items()) + ": "
          + ", ".join(f"{k} / other = {v / tot['other']:.4f}" for k, v in tot.items() if k != "other"), flush=True)
    del run, ys
    torch.cuda.empty_cache()
