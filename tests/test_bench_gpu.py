"""bench.py on the device: a plain run measures the headline alone, --full adds what takes runs of its own (kernel replay and roofline,
companions, fresh-tree variant, CPU baselines, c1_dropin), and both time the same steps on the same inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# a small headline workload (fp32-class evaluator, 2 x 128 tower) and a short --full protocol
SMALL = ["--gpus", "1", "--steps", "12", "--warmup", "2", "--games", "512", "--sims", "32", "--blocks", "2", "--preroll-rounds", "20",
         "--harvest-every", "6", "--cpu-seconds", "1", "--cpu-cores", "2"]
FULL_ONLY = ("roofline", "kernel_replay_range_events", "lower_precision_companion", "bf16_moves_per_s", "fp32_library_companion",
             "fp32_library_moves_per_s", "speedup_vs_library_fp32", "fresh_tree_companion", "fresh_tree_moves_per_s", "cpu_baseline",
             "speedup_vs_cpu_baseline", "speedup_vs_reference_equivalent_cpu", "c1_cpu_reference_path", "c1_dropin")


def _bench(extra, out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + extra + ["--dump-outputs", out_dir], env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    dumps = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in os.listdir(out_dir)}
    return json.loads(lines[0]), dumps


@pytest.mark.gpu
def test_gpu_bench_plain_run_is_the_headline_and_full_adds_the_rest(tmp_path):
    plain, plain_out = _bench([], str(tmp_path / "plain"))
    full, full_out = _bench(["--full"], str(tmp_path / "full"))
    for line in (plain, full):
        assert line["value"] > 0 and line["ms_per_step"] > 0 and line["unit"] == "moves/s" and line["higher_is_better"] is True
        assert line["dtype"].startswith("fp32-class evaluator") and line["evaluator_range_events"] == 0
        assert line["engine_roofline"]["avg_launch_ms"] > 0 and line["nn_roofline"]["avg_forward_ms"] > 0
    assert all(plain[k] is None for k in FULL_ONLY), {k: plain[k] for k in FULL_ONLY if plain[k] is not None}
    assert plain.keys() == full.keys()
    # --full: every measurement beside the headline ran
    assert "k_conv3x3_sp" in full["roofline"]["kernel"] and full["roofline"]["avg_launch_ms"] > 0 and full["kernel_replay_range_events"] == 0
    assert full["lower_precision_companion"]["moves_per_s"] > 0 and full["fp32_library_companion"]["moves_per_s"] > 0
    assert full["fresh_tree_companion"]["moves_per_s"] > 0 and full["cpu_baseline"]["value"] > 0 and full["c1_cpu_reference_path"]["value"] > 0
    assert "error" not in full["c1_dropin"] and full["c1_dropin"]["resident_eval_func_moves"] > 0
    # the same timed steps on the same inputs: identical work and identical outputs of the last timed step
    for k in ("preroll_rounds", "samples_gathered", "sims_per_move", "dup_leaf_rate", "terminal_hit_rate"):
        assert plain[k] == full[k], k
    assert plain_out.keys() == full_out.keys() and {"priors", "values", "status", "root_q", "samples_states"} <= plain_out.keys()
    for k in plain_out:
        assert np.array_equal(plain_out[k], full_out[k]), k
