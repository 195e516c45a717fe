"""Engine + REAL trained network vs the reference's uct_search + the same network (fixed seed: recorded Dirichlet draws / uniforms)."""
import json
import os

import pytest
import torch

import realnet_checks as rc


@pytest.mark.parametrize("name", ["gomoku13_ckpt200000_p1_s100", "gomoku13_ckpt200000_p1_s100_fresh", "gomoku13_ckpt200000_p8_s200"])
def test_host_twin_search_with_shipped_checkpoint_matches_reference_exactly(name):
    """CPU tier: the engine source (host twin) + the shipped checkpoint evaluated by torch-CPU fp32, the arithmetic the golden run used."""
    torch.set_num_threads(1)
    s = rc.check_exact("host", name)
    assert s["moves_compared"] >= 40


@pytest.mark.gpu
def test_gpu_search_with_shipped_checkpoint_fp32_and_bf16(golden_dir):
    """GPU tier.  (1) The HIP engine with the golden run's own evaluator arithmetic (fp32 torch-CPU module behind eval_func) equals the
    reference exactly.  (2) fp32 on the device (InferenceNet fp32: library convolutions + azsp_bias_act) differs from the CPU's fp32 in
    the last bits, so a PUCT arg-max can flip: teacher-forced on the reuse-free golden every move is an independent comparison; stated
    tolerance: >= 90 % of the moves identical (pi to 1e-6, same sampled move), all moves |pi - pi_ref|_inf <= 0.08, |root_Q - ref| <=
    0.02.  (3) bf16 hand-written kernels (checkpoint widened 40 -> 64 filters): reported, with loose bounds.  (4) the fp32-class
    hand-written evaluator (checkpoint widened to 64 filters, split-precision kernels on 17x17 planes): the bounds of (2).  """
    from alpha_zero_amd import _lib
    from alpha_zero_amd.core.network import InferenceNet, widen_network

    net = rc.load_shipped()
    out = {}
    for name in ("gomoku13_ckpt200000_p1_s100", "gomoku13_ckpt200000_p8_s200"):
        out["cpu_evaluator_" + name] = rc.check_exact("gpu", name)
    inf32 = InferenceNet(net, dtype=torch.float32, binding=_lib.load()).cuda()
    recs, total = rc.run_golden("gpu", "gomoku13_ckpt200000_p1_s100_fresh", rc.inference_eval_func(inf32, 13, tiled=False), teacher_forced=True)
    s32 = rc.summarize(recs, total)
    out["fp32_device_teacher_forced"] = s32
    inf16 = InferenceNet(widen_network(net, 64), dtype=torch.bfloat16, binding=_lib.load()).cuda()
    assert inf16.supports_tiled_features(13, "cuda")
    recs, total = rc.run_golden("gpu", "gomoku13_ckpt200000_p1_s100_fresh", rc.inference_eval_func(inf16, 13, tiled=True), teacher_forced=True)
    s16 = rc.summarize(recs, total)
    out["bf16_kernels_teacher_forced"] = s16
    recs, total = rc.run_golden("gpu", "gomoku13_ckpt200000_p1_s100", rc.inference_eval_func(inf32, 13, tiled=False), teacher_forced=False)
    out["fp32_device_free_run_with_reuse"] = rc.summarize(recs, total)
    assert "library" in inf32.evaluator_path(13, "cuda")  # (10 x 40: no hand-written kernel at this width -- that is what (4) widens for)
    # (4) round 4: the reference's precision class on HAND-WRITTEN kernels: the checkpoint widened 40 -> 64 filters (function-preserving)
    # on the split-precision evaluator (azsp_stem_split pad 3 -> azsp_conv3x3_split at 17x17 -> azsp_head_split).  Same statement and
    # bounds as the library fp32 path, on all three goldens (teacher-forced without reuse; free-running with reuse, P = 1 and P = 8).
    infsp = InferenceNet(widen_network(net, 64), dtype=torch.float32, binding=_lib.load()).cuda()
    assert "hand-written" in infsp.evaluator_path(13, "cuda") and "split-precision" in infsp.evaluator_path(13, "cuda")
    ssp = {}
    for key, name, tf in (("teacher_forced", "gomoku13_ckpt200000_p1_s100_fresh", True), ("free_run_with_reuse", "gomoku13_ckpt200000_p1_s100", False),
                          ("free_run_parallel_p8_s200", "gomoku13_ckpt200000_p8_s200", False)):
        infsp._split = None
        recs, total = rc.run_golden("gpu", name, rc.inference_eval_func(infsp, 13, tiled=False), teacher_forced=tf)
        assert infsp._split is not None, "the split-precision kernels did not run"
        ssp[key] = rc.summarize(recs, total)
    out["fp32_class_hand_written_kernels"] = ssp
    assert infsp.split_range_status(reset=True)[0] == 0
    os.makedirs(os.path.join(os.path.dirname(golden_dir), "..", "gpurun_out"), exist_ok=True)
    json.dump(out, open(os.path.join(os.path.dirname(golden_dir), "..", "gpurun_out", "realnet_search_parity.json"), "w"), indent=1)
    assert s32["moves_compared"] == s32["moves_in_golden"] >= 40
    assert s32["exact_moves"] >= 0.9 * s32["moves_compared"] and s32["max_dpi"] <= 0.08 and s32["max_dq"] <= 0.02, s32
    assert s16["same_move"] >= 0.8 and s16["top1"] >= 0.8 and s16["mean_dpi"] <= 0.05 and s16["mean_dq"] <= 0.03, s16
    # measured on MI355X (profiles/r04_realnet_search_parity.json): 54 / 54, 54 / 54 and 52 / 52 moves identical, pi identical, |dQ| <= 1.2e-7.
    # The hand-written kernels pick no algorithm at run time (unlike the library), so the statement is box-independent: EVERY move of
    # all three goldens identical (pi to 1e-6, same sampled move), |root_Q - ref| and |best_child_Q - ref| <= 1e-6.
    for key in ("teacher_forced", "free_run_with_reuse", "free_run_parallel_p8_s200"):
        f = ssp[key]
        assert f["moves_compared"] == f["moves_in_golden"] >= 40 and f["exact_moves"] == f["moves_compared"], ssp
        assert f["max_dpi"] <= 1e-6 and f["max_dq"] <= 1e-6 and f["max_dcq"] <= 1e-6, ssp


@pytest.mark.gpu
def test_gpu_dropin_search_with_the_device_resident_product_evaluator_reproduces_the_reference_games():
    """uct_search / parallel_uct_search handed a DeviceEvaluator (core/evaluate.py) around the fp32-class hand-written evaluator with the
    reference's shipped checkpoint: the leaves stay on the device, the forward is replayed from a hipGraph between the engine's own
    tensors, the host polls the status a few times per move.  Statement: the same as for the host callback -- EVERY move of the
    reference's recorded games identical (pi to 1e-6, same sampled move, |Q - ref| <= 1e-6), P = 1 with sub-tree reuse and P = 8.
    The P = 1 game is played once more after the P = 8 one with the same evaluator: a captured P = 1 forward that is replayed then must
    still own its scratch (every captured forward has a scratch slot of the network to itself: ADVICE r6 #1), so that leg is exact too."""
    from alpha_zero_amd import _lib
    from alpha_zero_amd.core.evaluate import DeviceEvaluator
    from alpha_zero_amd.core.network import InferenceNet, widen_network

    infsp = InferenceNet(widen_network(rc.load_shipped(), 64), dtype=torch.float32, binding=_lib.load()).cuda()
    for use_graph in (True, False):
        ev = DeviceEvaluator(infsp, use_graph=use_graph)
        for leg, name in enumerate(("gomoku13_ckpt200000_p1_s100", "gomoku13_ckpt200000_p8_s200", "gomoku13_ckpt200000_p1_s100")):
            infsp._split, captured = None, len(ev._graphs)
            recs, total = rc.run_golden("gpu", name, ev, teacher_forced=False)
            # (the third leg with graphs is all replays of the first leg's captures: no Python forward runs, nothing is captured anew)
            replays_only = use_graph and leg == 2 and len(ev._graphs) == captured
            assert infsp._split is not None or replays_only, "the split-precision kernels did not run"
            f = rc.summarize(recs, total)
            assert f["moves_compared"] == f["moves_in_golden"] >= 40 and f["exact_moves"] == f["moves_compared"], (use_graph, leg, name, f)
            assert f["max_dpi"] <= 1e-6 and f["max_dq"] <= 1e-6 and f["max_dcq"] <= 1e-6, (use_graph, leg, name, f)
            for _, slot in ev._graphs.values():  # every cached graph replays into scratch the network still holds
                assert ("split", slot) in infsp._scratch_cache, (use_graph, leg, name, slot)
        assert (len(ev._graphs) >= 1) == use_graph  # (one captured forward per engine buffer set)
    assert infsp.split_range_status(reset=True)[0] == 0
