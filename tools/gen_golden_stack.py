"""Golden vectors for observation history depths num_stack = K < 8, produced by IMPORTING the upstream reference (this container only).

Usage:  python tools/gen_golden_stack.py <task> [...]
Tasks:
  go_random N K [K ...]   seeded random-legal playouts on an NxN reference GoEnv(num_stack=K)  -> tests/golden/stack_goN_k<K>_random.npz
  gomoku N K [K ...]      seeded random playouts on a reference GomokuEnv(N, num_stack=K)       -> tests/golden/stack_gomokuN_k<K>_random.npz
  mcts NAME               search + actor golden in the gen_golden_mcts.py format               -> tests/golden/stack_mcts_<NAME>.npz
  all                     every file above, one child process per board size / config
The playout files hold the moves and per game a 16-byte digest of the env states and one of the 2K+1-plane observations
(tests/statehash.py).  Only derived DATA is written.  go_engine.py reads BOARD_SIZE at import time, so every board size runs in its
own process (`all` starts one child per task)."""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_harness  # noqa: E402
from statehash import TrajectoryHasher  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")

# MCTS / actor configs: gen_golden_mcts.py's keys plus num_stack
MCTS = {
    # the BASELINE shape at K = 4: 9-plane observations, parallel search, two games of about 40 moves
    "go9_p8_s200_k4": dict(game="go", n=9, sims=200, parallel=8, games=2, seed=51, resign_threshold=-1.0, resign_disabled=True, max_moves=40,
                           num_stack=4),
    # finished games on a tiny board: terminal leaves, and trees deeper than the 2-board history (ancestors vs real history in the planes)
    "go5_p4_s48_k2": dict(game="go", n=5, sims=48, parallel=4, games=3, seed=52, resign_threshold=-1.0, resign_disabled=True, num_stack=2),
    "gomoku13_p8_s200_k1": dict(game="gomoku", n=13, sims=200, parallel=8, games=2, seed=53, max_moves=40, num_stack=1),
}
PLAYOUTS = [("go_random", 9, (1, 4), 60), ("go_random", 19, (2,), 12), ("gomoku", 13, (1, 4), 60)]


def _hash_game(env, moves, record):
    h = TrajectoryHasher()
    obs = env.reset()
    assert obs.shape[0] == 2 * env.num_stack + 1
    h.add(record(env, False, 0), obs)
    for a in moves:
        obs, reward, done, _ = env.step(int(a))
        h.add(record(env, done, reward), obs)
    return h.digests()


def _save(name, moves_per_game, digests, **extra):
    offsets = np.cumsum([0] + [len(m) for m in moves_per_game]).astype(np.int32)
    np.savez_compressed(os.path.join(GOLD, name), moves=np.array([a for m in moves_per_game for a in m], dtype=np.uint16), offsets=offsets,
                        state_digest=np.stack([np.frombuffer(d[0], dtype=np.uint8) for d in digests]),
                        obs_digest=np.stack([np.frombuffer(d[1], dtype=np.uint8) for d in digests]), **extra)
    print(f"{name}: {len(moves_per_game)} games, {int(offsets[-1])} moves")


def task_go_random(n, ks, games, seed=4321):
    ref_harness.install(n)
    from alpha_zero.envs.go import GoEnv
    from gen_golden import go_record, random_go_game

    for k in ks:
        rng = np.random.Generator(np.random.PCG64(seed + 100 * n + k))
        env = GoEnv(num_stack=k)
        lists = [random_go_game(env, rng, 0.0 if g % 3 == 0 else 0.03) for g in range(games)]
        _save(f"stack_go{n}_k{k}_random.npz", lists, [_hash_game(env, m, go_record) for m in lists])


def task_gomoku(n, ks, games, seed=8765):
    ref_harness.install(9)
    from alpha_zero.envs.gomoku import GomokuEnv
    from gen_golden import gomoku_record

    for k in ks:
        rng = np.random.Generator(np.random.PCG64(seed + 100 * n + k))
        env = GomokuEnv(board_size=n, num_stack=k)
        lists = []
        for _ in range(games):
            env.reset()
            moves, done = [], False
            while not done:
                legal = np.flatnonzero(env.legal_actions)
                a = int(legal[rng.integers(len(legal))])
                _, _, done, _ = env.step(a)
                moves.append(a)
            lists.append(moves)
        _save(f"stack_gomoku{n}_k{k}_random.npz", lists, [_hash_game(env, m, gomoku_record) for m in lists])


def task_mcts(name):
    import gen_golden_mcts

    gen_golden_mcts.main(name, MCTS[name], os.path.join(GOLD, f"stack_mcts_{name}.npz"))


def main(argv):
    task = argv[0]
    if task == "go_random":
        task_go_random(int(argv[1]), [int(k) for k in argv[2:]], dict((p[1], p[3]) for p in PLAYOUTS if p[0] == "go_random")[int(argv[1])])
    elif task == "gomoku":
        task_gomoku(int(argv[1]), [int(k) for k in argv[2:]], dict((p[1], p[3]) for p in PLAYOUTS if p[0] == "gomoku")[int(argv[1])])
    elif task == "mcts":
        task_mcts(argv[1])
    elif task == "all":
        jobs = [[t, str(n)] + [str(k) for k in ks] for t, n, ks, _ in PLAYOUTS] + [["mcts", name] for name in MCTS]
        for j in jobs:  # one process per board size / config: BOARD_SIZE is read when the reference's go_engine is imported
            subprocess.check_call([sys.executable, os.path.abspath(__file__)] + j)
    else:
        raise SystemExit(__doc__)


if __name__ == "__main__":
    main(sys.argv[1:])
