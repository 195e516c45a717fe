"""What the Gumbel root search (SelfPlayActor(gumbel=m)) costs an actor, off and on.

Off against the parent commit: `--parent DIR` names a built checkout of the parent commit.  `python bench.py --gpus 1 --steps S
--warmup W` -- the headline workload, the mode off -- then runs `--pairs` times in each tree, in fresh processes, alternating
(parent, child, parent, child, ...; `--child-first` swaps the order inside a pair).  Printed: moves/s and the select launch's mean time
of every run in the order they ran, the parent's spread (max - min over its runs), and child - parent pair by pair.  The off path may be
slower than the parent by no more than that spread.

On against off, on this build: the headline shape of bench.py (9x9 Go, 4096 games, 200 simulations, 8 leaves per round, 10 x 128
network, fp32-class evaluator) twice with the same staggered openings and the same number of untimed and timed rounds: once with the
mode off and once with gumbel=m.  Every timed round is bracketed by events: moves/s, sims/s and the mean time of the select kernel (where
the considered action is chosen in front of every descent), of expand / backup + end of move (where the base row, a* and pi' are formed)
and of the forward.  The two runs search differently, so the rates are those of two different, equally long workloads.

    python tools/gumbel_rate.py [--parent DIR --pairs 3] [--m 16] [--steps 300] [--preroll 200]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from alpha_zero_amd.core.network import AlphaZeroNet  # noqa: E402
from alpha_zero_amd.core.pipeline import SelfPlayActor  # noqa: E402


def bench_line(tree, steps, warmup):
    """The result line of one `bench.py` run in `tree` (a process of its own)."""
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--no-cpu-baseline",
                          "--no-companions", "--no-fresh-tree"], cwd=tree, capture_output=True, text=True, check=True, timeout=600).stdout
    for row in reversed(out.strip().split("\n")):
        if row.startswith("{") and '"value"' in row:
            return json.loads(row)
    raise SystemExit("no result line from bench.py in " + tree)


def off_against_parent(args):
    runs = []
    order = [("child", ROOT), ("parent", args.parent)] if args.child_first else [("parent", args.parent), ("child", ROOT)]
    for _ in range(args.pairs):
        for who, tree in order:
            line = bench_line(tree, args.bench_steps, args.bench_warmup)
            runs.append(dict(build=who, moves_per_s=line["value"], serial_step_ms=line.get("serial_step_ms")))
            print(json.dumps(runs[-1]), flush=True)
    par = [r["moves_per_s"] for r in runs if r["build"] == "parent"]
    chi = [r["moves_per_s"] for r in runs if r["build"] == "child"]
    spread = max(par) - min(par)
    print(json.dumps(dict(off_against_parent=dict(parent=par, child=chi, parent_spread=round(spread, 2),
                                                  child_minus_parent=[round(c - p, 2) for c, p in zip(chi, par)],
                                                  mean_child_minus_parent=round(float(np.mean(chi) - np.mean(par)), 2),
                                                  within_parent_spread=bool(np.mean(chi) >= np.mean(par) - spread)))), flush=True)


def run(args, m):
    n, dev = args.board, torch.device("cuda")
    torch.manual_seed(1)
    net = AlphaZeroNet((17, n, n), n * n + 1, args.blocks, args.filters, args.filters)
    act = SelfPlayActor(net, game="go", board_size=n, num_games=args.games, num_simulations=args.sims, num_parallel=args.parallel,
                        warm_up_steps=16, resign_threshold=-1.0, seed=1, device=dev, net_dtype=torch.float32, gumbel=m)
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
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for i in range(args.steps):
        act.run_round(evs[i])
        if (i + 1) % args.harvest_every == 0:
            act.harvest_tensors()
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    cnt = act.counters()
    phase = lambda a: round(float(np.mean([ev[a].elapsed_time(ev[a + 1]) for ev in evs])) * 1e3, 1)  # noqa: E731  (microseconds)
    res = dict(gumbel=m, rounds=args.steps, seconds=round(dt, 3), moves_per_s=round(cnt["moves"] / dt, 1), sims_per_s=round(cnt["sims"] / dt, 1),
               backup_endmove_us=phase(0), select_us=phase(1), forward_us=phase(2), range_events=act.range_events, evaluator=act.evaluator_path)
    e.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: bench.py runs there and here, alternating")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--child-first", action="store_true")
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=5)
    ap.add_argument("--no-on", action="store_true", help="only the off path against the parent")
    ap.add_argument("--m", type=int, default=16, help="considered actions of the on run")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--preroll", type=int, default=200)
    ap.add_argument("--harvest-every", type=int, default=50)
    ap.add_argument("--stagger", type=int, default=60)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--board", type=int, default=9)
    ap.add_argument("--sims", type=int, default=200)
    ap.add_argument("--parallel", type=int, default=8)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--filters", type=int, default=128)
    args = ap.parse_args()
    if args.parent:
        off_against_parent(args)
    if args.no_on:
        return
    off = run(args, None)
    print(json.dumps(off), flush=True)
    on = run(args, args.m)
    print(json.dumps(on), flush=True)
    ratio = lambda key: round(on[key] / off[key], 4) if off[key] else None  # noqa: E731
    print(json.dumps(dict(on_over_off={key: ratio(key) for key in ("moves_per_s", "sims_per_s", "select_us", "backup_endmove_us", "forward_us")})))


if __name__ == "__main__":
    main()
