"""Searches per second of n positions searched at once (uct_search_many) against n sequential uct_search calls, with the same
DeviceEvaluator (fp32-class InferenceNet, seeded random weights): python tools/batch_search_rate.py --n 64 --sims 100
Prints one JSON line.  The positions are random openings of different lengths; both legs search the same positions from fresh roots
(deterministic arg-max moves, no root noise), so they also must return the same moves."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--game", default="gomoku")
    ap.add_argument("--board", type=int, default=13)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--parallel", type=int, default=1)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--filters", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    from alpha_zero_amd import _lib
    from alpha_zero_amd.core.evaluate import DeviceEvaluator
    from alpha_zero_amd.core.mcts_v2 import parallel_uct_search, parallel_uct_search_many
    from alpha_zero_amd.core.network import AlphaZeroNet, InferenceNet
    from alpha_zero_amd.envs.go import GoEnv
    from alpha_zero_amd.envs.gomoku import GomokuEnv

    torch.manual_seed(0)
    go = a.game == "go"
    A = a.board ** 2 + (1 if go else 0)
    net = AlphaZeroNet((17, a.board, a.board), A, a.blocks, a.filters, 64, gomoku=not go).eval()
    ev = DeviceEvaluator(InferenceNet(net, dtype=torch.float32, binding=_lib.load()).cuda())
    rng = np.random.Generator(np.random.PCG64(1))
    envs = []
    for i in range(a.n):
        env = GoEnv(board_size=a.board) if go else GomokuEnv(board_size=a.board)
        for _ in range(2 + i % 17):
            legal = np.flatnonzero(env.legal_actions[: a.board ** 2])
            env.step(int(legal[rng.integers(len(legal))]))
        envs.append(env)
    kw = dict(c_puct_base=19652.0, c_puct_init=1.25, num_simulations=a.sims, num_parallel=a.parallel, deterministic=True)

    def sequential():
        return [int(parallel_uct_search(env, ev, None, **kw)[0]) for env in envs]

    def batched():
        return [int(m) for m in parallel_uct_search_many(envs, ev, None, **kw)[0]]

    out = {}
    for name, f in (("sequential", sequential), ("batched", batched)):
        moves = f()  # warm-up: engines, graph captures
        best = float("inf")
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            t = time.perf_counter()
            f()
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t)
        out[name] = dict(seconds=round(best, 4), searches_per_s=round(a.n / best, 1), moves=moves)
    same = out["sequential"].pop("moves") == out["batched"].pop("moves")
    print(json.dumps(dict(game=a.game, board=a.board, n=a.n, sims=a.sims, parallel=a.parallel, blocks=a.blocks, filters=a.filters, same_moves=same,
                          speedup=round(out["sequential"]["seconds"] / out["batched"]["seconds"], 2), **out)))


if __name__ == "__main__":
    main()
