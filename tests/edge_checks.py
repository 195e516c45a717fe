"""The reference's known-answer edge cases through the engine's env kernels (azsp_env_step / azsp_set_state), shared by the CPU
tier (host twin) and the GPU tier (libazsp.so):
  * unit_tests/envs/go_test.py:80-209 (19x19): two suicide shapes, ko, the two scoring sequences, the stacked planes -- golden
    go19_known.npz (boards / legal masks / observations / rewards recorded from the reference's GoEnv, tools/gen_golden.py);
  * others/go_score_system.py:100-236: the 7 hand-made 9x9 boards and the areas the reference's area_score returns --
    golden go9_score_boards.npz."""
import os

import numpy as np
import pytest

import dropin_checks as dc
import engine_util as eu
from alpha_zero_amd import _abi


def check_go19_known_sequences(kind, golden_dir):
    g = np.load(os.path.join(golden_dir, "go19_known.npz"))
    names = [str(x) for x in g["names"]]
    assert len(names) >= 5
    for name in names:
        env = dc.make_env(kind, "go", 19)
        env.reset()
        reward, done = 0.0, False
        for a in g[f"{name}__moves"]:
            _, reward, done, _ = env.step(int(a))
        assert bool(g[f"{name}__done"]) == done and float(g[f"{name}__reward"]) == reward, name
        assert int(g[f"{name}__winner"]) == (env.winner or 0), name
        assert np.array_equal(g[f"{name}__legal"], np.asarray(env.legal_actions).astype(np.int8)), name
        assert np.array_equal(g[f"{name}__board"], np.asarray(env.board).ravel()), name
        assert np.array_equal(g[f"{name}__obs"], env.observation()), name
        if f"{name}__probe" in g:  # the move the reference test expects to be refused (suicide / ko recapture)
            assert int(g[f"{name}__probe_legal"]) == 0
            assert env.legal_actions[int(g[f"{name}__probe"])] == 0
            before = np.asarray(env.board).copy()
            with pytest.raises(ValueError, match="Illegal action"):
                env.step(int(g[f"{name}__probe"]))
            assert np.array_equal(before, np.asarray(env.board))  # a refused move leaves the position untouched
    assert int(g["score_black__winner"]) == 1 and int(g["score_white__winner"]) == -1


def check_go9_score_boards(kind, golden_dir):
    """Each board is loaded with azsp_set_state; two passes end the game and the env kernel scores it (go_engine.py:123-152
    area_score, :527-534 result).  Areas, winner and reward must equal the reference's values for the same board."""
    from alpha_zero_amd.core.engine import Engine, EngineConfig

    g = np.load(os.path.join(golden_dir, "go9_score_boards.npz"))
    boards, areas = g["boards"], g["areas"]
    assert len(boards) == 7
    binding, dev = eu.backend(kind)
    eng = Engine(binding, EngineConfig(game="go", board_size=9, num_games=len(boards), num_parallel=1, num_simulations=2, stop_after_move=True),
                 device=dev)
    for i, b in enumerate(boards):
        b8 = np.ascontiguousarray(b, dtype=np.int8)
        hist = np.zeros((8, 81), dtype=np.int8)
        hist[0] = b8.ravel()
        eng.set_state(i, b8, hist, to_play=1, steps=30)
    out = eng.env_step(None)
    assert np.array_equal(out["board"].reshape(len(boards), 81), boards.reshape(len(boards), 81).astype(np.int8))
    eng.env_step(np.full(len(boards), 81, dtype=np.int32))          # black passes
    out = eng.env_step(np.full(len(boards), 81, dtype=np.int32))    # white passes: game over, scored
    sc = out["scalars"]
    for i, (eb, ew) in enumerate(areas):
        assert sc[i, _abi.ENV_DONE] == 1 and (sc[i, _abi.ENV_AREA_BLACK], sc[i, _abi.ENV_AREA_WHITE]) == (eb, ew), (i, sc[i], eb, ew)
        diff = float(eb) - (float(ew) + 7.5)
        winner = 1 if diff > 0 else -1
        assert sc[i, _abi.ENV_WINNER] == winner
        # reward is from the last mover's (white's) point of view (go.py:141-150)
        assert sc[i, _abi.ENV_REWARD] == (1 if winner == -1 else -1)
    eng.close()
