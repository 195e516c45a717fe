"""What the playout cap (SelfPlayActor(playout_cap=...), DESIGN "Per-game budgets and the playout cap") does to an actor's rates.

Runs the headline shape of bench.py (9x9 Go, 4096 games, 200 simulations, 8 leaves per round, 10 x 128 network, fp32-class
evaluator) twice on the same build, with the same staggered openings and the same number of untimed and timed rounds: once with the
cap off -- the yardstick -- and once with the cap on, by default (40, 0.25).  Prints one JSON line per run and one with the ratios:
moves/s (every searched move), samples/s (every recorded sample) and full samples/s (the samples a learner is handed: all of them with
the cap off, the full-search ones with it on).  Samples are counted when their game is harvested, and a timed window of a few hundred
rounds is shorter than a game, so the sample and game rates of a run depend on how many games happen to end inside the window; moves/s
and sims/s do not.  full_moves_per_s = moves/s x the full fraction of the harvested samples is the rate at which full-search samples are
PRODUCED, whenever their games end.

    python tools/playout_cap_rate.py [--fast 40] [--full-prob 0.25] [--steps 400] [--preroll 300]
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


def run(args, cap):
    n, dev = args.board, torch.device("cuda")
    torch.manual_seed(1)
    net = AlphaZeroNet((17, n, n), n * n + 1, args.blocks, args.filters, args.filters)
    act = SelfPlayActor(net, game="go", board_size=n, num_games=args.games, num_simulations=args.sims, num_parallel=args.parallel,
                        warm_up_steps=16, resign_threshold=-1.0, seed=1, device=dev, net_dtype=torch.float32, playout_cap=cap)
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
    torch.cuda.synchronize(dev)
    samples = full = games = 0
    t0 = time.perf_counter()
    for i in range(args.steps):
        act.run_round()
        if (i + 1) % args.harvest_every == 0:
            _, _, z, rows = act.harvest_tensors()
            samples, games, full = samples + int(z.shape[0]), games + len(rows), full + int(act.last_harvest_full.sum().item())
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    cnt = act.counters()
    res = dict(playout_cap=list(cap) if cap else None, rounds=args.steps, seconds=round(dt, 3), moves_per_s=round(cnt["moves"] / dt, 1),
               sims_per_s=round(cnt["sims"] / dt, 1), samples_per_s=round(samples / dt, 1), full_samples_per_s=round(full / dt, 1),
               full_fraction=round(full / max(1, samples), 4), full_moves_per_s=round(cnt["moves"] / dt * full / max(1, samples), 1),
               games_per_s=round(games / dt, 2), sims_per_move=round(cnt["sims"] / max(1, cnt["moves"]), 1), evaluator=act.evaluator_path)
    e.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fast", type=int, default=40)
    ap.add_argument("--full-prob", type=float, default=0.25)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--preroll", type=int, default=300)
    ap.add_argument("--harvest-every", type=int, default=50)
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
    on = run(args, (args.fast, args.full_prob))
    print(json.dumps(on), flush=True)
    ratio = lambda k: round(on[k] / off[k], 3) if off[k] else None  # noqa: E731
    print(json.dumps(dict(cap_on_over_cap_off={k: ratio(k) for k in ("moves_per_s", "full_moves_per_s", "samples_per_s", "full_samples_per_s", "games_per_s")})))


if __name__ == "__main__":
    main()
