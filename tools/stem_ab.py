"""Same-box A/B of the wave-per-tile fp32-class stem k_stem_spg (csrc/az_conv_spg.h) and of the opt-in whole evaluator built on it
(InferenceNet.use_split_any_board), alternating runs:
  (a) the stem alone on the three tailored shapes, tailored kernel (azsp_small_batch_waves(0)) against wave-per-tile (a huge threshold),
      at 1, 8, 16 and 64 boards: decides whether the default threshold moves the tailored shapes (azsp_hip.hip STEM_SPG_DEFAULT_SMALL);
  (b) the whole forward at 19x19 x {64, 128, 256}, switch off against on, at 1, 8, 256 and 2048 rows, fed fp32 planes and -- where the
      switch allows -- an engine-written AZSP_FEAT_F16_SPLIT tensor.
usage: python tools/stem_ab.py [--part a|b|ab] [--filters 64,128,256]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

from alpha_zero_amd import _lib
from alpha_zero_amd.core.network import AlphaZeroNet, InferenceNet, split_weights_f16

ap = argparse.ArgumentParser()
ap.add_argument("--part", default="ab")
ap.add_argument("--filters", default="64,128,256")
args = ap.parse_args()
dll = _lib.load().dll
dev = "cuda"
HUGE = 1 << 40


def timed(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3  # us


def alternate(fns, reps, rounds=5):
    """fns: name -> callable; `rounds` alternating timings of each: [median, min, max] per name (us per call, back-to-back calls from
    Python between two device events: for kernels of a few microseconds this is the rate of launches, the figure a forward pays)."""
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ts[k].append(timed(fn, reps))
    return {k: [round(sorted(v)[len(v) // 2], 2), round(min(v), 2), round(max(v), 2)] for k, v in ts.items()}


old = dll.azsp_small_batch_waves(-1)
out = {"default_small_batch_waves": old}
if "a" in args.part:
    out["stem_us"] = {}
    for n, pad, C in ((9, 1, 128), (9, 1, 64), (13, 3, 64)):
        S = n + 2 * (pad - 1)
        for B in (1, 8, 16, 64):
            g = torch.Generator().manual_seed(B)
            x = (torch.rand(B, 17, n, n, generator=g) > 0.6).float().to(dev)
            feat = torch.zeros(dll.azsp_split_bytes(B, n, 32) // 2, dtype=torch.float16, device=dev)
            ys = torch.zeros(dll.azsp_split_bytes(B, S, C) // 2, dtype=torch.float16, device=dev)
            assert dll.azsp_split_features(x.data_ptr(), feat.data_ptr(), B, n, 17, None, None) == 0
            w32 = torch.zeros(C, 32, 3, 3)
            w32[:, :17] = torch.randn(C, 17, 3, 3, generator=g) * 0.1
            w, b = split_weights_f16(w32).to(dev), (torch.randn(C, generator=g) * 0.1).to(dev)
            res = {}
            for name, entry in (("general", dll.azsp_stem_split), ("exact", dll.azsp_stem_split_exact)):

                def run(thr, entry=entry):
                    dll.azsp_small_batch_waves(thr)
                    assert entry(feat.data_ptr(), w.data_ptr(), b.data_ptr(), ys.data_ptr(), B, n, C, pad, 1, None, None) == 0

                t = alternate({"tailored": lambda: run(0), "wave_per_tile": lambda: run(HUGE)}, 200)
                res[name] = t
            out["stem_us"][f"{n}x{n} pad={pad} C={C} boards={B}"] = res
            print(n, pad, C, B, res, flush=True)
    dll.azsp_small_batch_waves(old)
if "b" in args.part:
    import engine_util as eu

    out["forward_19x19_us"] = {}
    for C in (int(f) for f in args.filters.split(",")):
        torch.manual_seed(0)
        inf = InferenceNet(AlphaZeroNet((17, 19, 19), 362, 2, C, 256).eval(), dtype=torch.float32, binding=_lib.load()).to(dev)
        for B in (1, 8, 256, 2048):
            x = (torch.rand(B, 17, 19, 19, generator=torch.Generator().manual_seed(B)) > 0.6).float()
            xd, xs = x.to(dev), eu.split_features(x).to(dev)
            pri, val = torch.empty(B, 362, device=dev), torch.empty(B, device=dev)

            def fwd(on, split):
                inf.use_split_any_board = on
                if split:
                    inf.forward_rows(xs, "split", B, 19, pri, val)
                else:
                    inf.forward(xd, pri, val)

            fwd(True, True)  # (calibration, scratch)
            t = alternate({"off_fp32_planes": lambda: fwd(False, False), "on_fp32_planes": lambda: fwd(True, False),
                           "on_engine_split_features": lambda: fwd(True, True)}, 50 if B <= 256 else 10)
            out["forward_19x19_us"][f"2 blocks x {C} rows={B}"] = t
            print(C, B, t, flush=True)
        del inf
print(json.dumps(out))
