"""Helpers shared by the oracle / host-twin / GPU search-parity tests: load an MCTS golden file
(produced by the reference, tools/gen_golden_mcts.py; the stack_mcts_* family at num_stack < 8 by tools/gen_golden_stack.py) and expose
its per-move records."""
import glob
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def names(real_network=False):
    """Goldens recorded with the synthetic hash evaluator (tests/synth_eval.py), or (real_network=True) the ones recorded with the
    reference's shipped checkpoint as evaluator (tests/realnet_checks.py)."""
    return sorted(n for n in (os.path.basename(f)[5:-4] for f in glob.glob(os.path.join(GOLDEN, "mcts_*.npz"))) if ("ckpt" in n) == real_network)


class MctsGolden:
    def __init__(self, name, prefix="mcts_"):
        self.g = np.load(os.path.join(GOLDEN, f"{prefix}{name}.npz"))
        self.cfg = json.loads(str(self.g["config"]))
        self.A, self.K = self.cfg["num_actions"], self.cfg.get("num_stack", 8)

    def moves_of_game(self, gi):
        return np.flatnonzero(self.g["game"] == gi)

    def finished(self, gi):
        return bool(int(self.g[f"g{gi}_finished"]))

    def samples(self, gi):
        n, C = self.cfg["n"], 2 * self.K + 1
        st = np.unpackbits(self.g[f"g{gi}_states"], axis=1)[:, : C * n * n].reshape(-1, C, n, n).astype(np.int8)
        return st, self.g[f"g{gi}_pis"], self.g[f"g{gi}_zs"], json.loads(str(self.g[f"g{gi}_stats"]))
