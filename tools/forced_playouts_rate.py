"""What forced playouts with policy-target pruning (SelfPlayActor(forced_playouts=k)) cost an actor.

Runs the headline shape of bench.py (9x9 Go, 4096 games, 200 simulations, 8 leaves per round, 10 x 128 network, fp32-class
evaluator) twice on the same build, with the same staggered openings and the same number of untimed and timed rounds: once with the
rule off -- the yardstick -- and once with forced_playouts=k.  Every timed round is bracketed by events, so besides moves/s and sims/s
each run reports the mean time of the select kernel (where the forced test runs in front of every descent), of expand / backup + end of
move (where the target is pruned) and of the forward.  Both runs log the last search of every slot (one log row per slot), so the on
run can compare, every `--sample-every` rounds, each slot's target row with the unpruned policy of the same search: the share of
searches whose target pruning changed.  Prints one JSON line per run and one with the ratios.  The searches of the two runs differ
(forcing changes what is selected), so the rates are those of two different, equally long workloads, not of one workload timed twice.

    python tools/forced_playouts_rate.py [--k 2] [--steps 300] [--preroll 200]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from alpha_zero_amd.core.network import AlphaZeroNet  # noqa: E402
from alpha_zero_amd.core.pipeline import SelfPlayActor  # noqa: E402


def run(args, k):
    n, dev = args.board, torch.device("cuda")
    torch.manual_seed(1)
    net = AlphaZeroNet((17, n, n), n * n + 1, args.blocks, args.filters, args.filters)
    act = SelfPlayActor(net, game="go", board_size=n, num_games=args.games, num_simulations=args.sims, num_parallel=args.parallel,
                        warm_up_steps=16, resign_threshold=-1.0, seed=1, device=dev, net_dtype=torch.float32, forced_playouts=k,
                        engine_kw=dict(log_moves=True, log_capacity=1))  # one log row per slot: its last finished search
    e = act.engine
    rng = np.random.Generator(np.random.PCG64(1234))  # the staggered openings of bench.py: mixed game phases from the first round
    plies = rng.integers(0, args.stagger + 1, size=args.games)
    out = e.env_step(None)
    for t in range(int(plies.max())):
        legal = out["legal"][:, : n * n].astype(bool)
        r = rng.random(legal.shape) * legal
        acts = np.where((plies > t) & legal.any(axis=1) & (out["scalars"][:, 5] == 0), r.argmax(axis=1), -2).astype(np.int32)
        out = e.env_step(acts)
    for i in range(args.preroll):
        act.run_round()
        if (i + 1) % args.harvest_every == 0:
            act.harvest_tensors()
    act.harvest_tensors()
    act.counters(reset=True)
    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(args.steps)]
    searched = changed = 0
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for i in range(args.steps):
        act.run_round(evs[i])
        if (i + 1) % args.harvest_every == 0:
            act.harvest_tensors()
        if k and (i + 1) % args.sample_every == 0:  # (device tensors; the two sums are read after the clock stops)
            pi, target = e.read_searches()[0], e.target_policies()
            done = target.sum(1) > 0
            searched = searched + done.sum()
            changed = changed + (done & (target != pi).any(1)).sum()
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    cnt = act.counters()
    phase = lambda a: round(float(np.mean([ev[a].elapsed_time(ev[a + 1]) for ev in evs])) * 1e3, 1)  # noqa: E731  (microseconds)
    res = dict(forced_playouts=k, rounds=args.steps, seconds=round(dt, 3), moves_per_s=round(cnt["moves"] / dt, 1),
               sims_per_s=round(cnt["sims"] / dt, 1), backup_endmove_us=phase(0), select_us=phase(1), forward_us=phase(2),
               searches_sampled=int(searched), targets_changed_by_pruning=int(changed),
               share_changed=round(int(changed) / int(searched), 4) if int(searched) else None,
               range_events=act.range_events, evaluator=act.evaluator_path)
    e.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=float, default=2.0, help="the forcing factor (KataGo: 2)")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--preroll", type=int, default=200)
    ap.add_argument("--harvest-every", type=int, default=50)
    ap.add_argument("--sample-every", type=int, default=25)
    ap.add_argument("--stagger", type=int, default=60)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--board", type=int, default=9)
    ap.add_argument("--sims", type=int, default=200)
    ap.add_argument("--parallel", type=int, default=8)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--filters", type=int, default=128)
    args = ap.parse_args()
    off = run(args, None)
    print(json.dumps(off), flush=True)
    on = run(args, args.k)
    print(json.dumps(on), flush=True)
    ratio = lambda key: round(on[key] / off[key], 4) if off[key] else None  # noqa: E731
    print(json.dumps(dict(on_over_off={key: ratio(key) for key in ("moves_per_s", "sims_per_s", "select_us", "backup_endmove_us", "forward_us")})))


if __name__ == "__main__":
    main()
