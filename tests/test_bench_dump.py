"""bench.py --dump-outputs without a GPU: bench.py's own timed region on a host-twin actor runs exactly --steps rounds, and what
step_outputs / dump_outputs write after it is float32 / float64, identical from run to run and within the size budget."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _run(steps, out_dir):
    import bench
    import engine_util as eu
    from alpha_zero_amd.core.network import AlphaZeroNet
    from alpha_zero_amd.core.pipeline import SelfPlayActor

    torch.manual_seed(1)
    net = AlphaZeroNet((17, 5, 5), 26, 1, 8, 8)
    act = SelfPlayActor(net, game="go", board_size=5, num_games=16, num_simulations=12, num_parallel=4, warm_up_steps=4, device="cpu",
                        net_dtype=torch.float32, use_graph=False, binding=eu.hosttwin_binding(), seed=1)
    args = argparse.Namespace(preroll_rounds=80, preroll_moves=2, harvest_every=7, sims=12, parallel=4)
    dev = torch.device("cpu")
    bench.preroll(act, args, 1, dev)  # 80 rounds: games finish from here on, so the timed region's harvests carry samples
    r0 = act.rounds
    bench.timed(act, args, 1, dev, warmup=3, steps=steps)
    assert act.rounds - r0 == 3 + steps  # --warmup then exactly --steps rounds
    paths = bench.dump_outputs(out_dir, bench.step_outputs(act))
    return {os.path.basename(p)[:-4]: np.load(p) for p in paths}


def test_dump_outputs_of_the_timed_path_are_reproducible(tmp_path):
    a = _run(20, str(tmp_path / "a"))
    b = _run(20, str(tmp_path / "b"))
    assert set(a) == set(b) == {"priors", "values", "status", "root_q", "samples_states", "samples_pi", "samples_z", "samples_games"}
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
    assert a["priors"].shape == (64, 26) and a["values"].shape == (64,) and a["status"].shape == (16, 8) and a["root_q"].shape == (16, 2)
    n = a["samples_states"].shape[0]
    assert n > 0 and a["samples_pi"].shape == (n, 26) and a["samples_z"].shape == (n,)
    assert np.allclose(a["samples_pi"].sum(1), 1.0, atol=1e-5) and set(np.unique(a["samples_states"])) <= {0.0, 1.0}
    c = _run(21, str(tmp_path / "c"))  # one more timed step: a different last step
    assert not all(np.array_equal(a[k], c[k]) for k in ("priors", "status", "root_q"))


def test_dump_outputs_keeps_a_seeded_row_sample_within_the_budget(tmp_path):
    import bench

    rng = np.random.default_rng(3)
    arrays = {"priors": rng.random((5000, 82), dtype=np.float32), "values": rng.random(5000, dtype=np.float32),
              "status": rng.random((700, 8))}
    budget = 600_000
    paths = bench.dump_outputs(str(tmp_path / "a"), arrays, budget=budget)
    assert sum(os.path.getsize(p) for p in paths) <= budget
    got = {os.path.basename(p)[:-4]: np.load(p) for p in paths}
    assert set(got) == {"priors", "values", "status", "priors_rows", "values_rows", "status_rows"}
    assert np.array_equal(got["priors_rows"], got["values_rows"])  # equal row counts keep the same rows: priors and values stay paired
    for k in arrays:
        rows = got[k + "_rows"].astype(np.int64)
        assert got[k + "_rows"].dtype == np.float64 and 0 < len(rows) < len(arrays[k]) and np.array_equal(got[k], arrays[k][rows])
    again = bench.dump_outputs(str(tmp_path / "b"), arrays, budget=budget)
    assert all(np.array_equal(np.load(p), np.load(q)) for p, q in zip(paths, again))
    small = bench.dump_outputs(str(tmp_path / "c"), {"values": arrays["values"]})  # under the budget: written whole, no row list
    assert [os.path.basename(p) for p in small] == ["values.npy"] and np.array_equal(np.load(small[0]), arrays["values"])
