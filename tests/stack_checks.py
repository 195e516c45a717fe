"""Cases and assertions of the num_stack tests (observation history depth K = 1..8, 2K+1 planes), shared by the host twin
(tests/test_num_stack_host.py) and the GPU (tests/test_num_stack_gpu.py).  The goldens (tests/golden/stack_*.npz) come from the
reference at K < 8 (tools/gen_golden_stack.py)."""
import os

import numpy as np

import engine_util as eu
from alpha_zero_amd import _abi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PLAYOUTS = [("go", 9, 1), ("go", 9, 4), ("go", 19, 2), ("gomoku", 13, 1), ("gomoku", 13, 4)]
MCTS_PREFIX = "stack_mcts_"  # golden_mcts.MctsGolden(name, MCTS_PREFIX)
MCTS = ["go9_p8_s200_k4", "go5_p4_s48_k2", "gomoku13_p8_s200_k1"]
FEATS = {"i8": _abi.FEAT_I8, "f32": _abi.FEAT_F32, "bf16": _abi.FEAT_BF16_TILED, "f16": _abi.FEAT_F16_TILED, "f16_split": _abi.FEAT_F16_SPLIT}


def check_playouts(kind, game, n, k):
    g = np.load(os.path.join(GOLDEN, f"stack_{game}{n}_k{k}_random.npz"))
    off, mv = g["offsets"], g["moves"]
    lists = [mv[off[i]:off[i + 1]].astype(np.int32) for i in range(len(off) - 1)]
    played, ds, do, _ = eu.replay_env_batch(kind, game, n, lists, num_stack=k)
    bad = [i for i in range(len(lists)) if played[i] != len(lists[i]) or ds[i] != g["state_digest"][i].tobytes()
           or do[i] != g["obs_digest"][i].tobytes()]
    assert len(lists) > 0 and not bad, bad[:5]
