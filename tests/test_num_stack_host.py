"""CPU tier of the observation history depth num_stack = K (1..8, 2K+1 planes): the engine source compiled as the host twin
(tests/hosttwin) against the reference's playouts and search / actor goldens at K < 8 (tools/gen_golden_stack.py), the limits of
the setting, and the two-rank sample gather of 2K+1-plane samples."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import engine_util as eu
import parity_checks as pc
import stack_checks as sc
from alpha_zero_amd import _abi
from alpha_zero_amd.core.engine import Engine, EngineConfig


@pytest.mark.parametrize("game,n,k", sc.PLAYOUTS)
def test_playouts_match_reference(game, n, k):
    sc.check_playouts("host", game, n, k)


@pytest.mark.parametrize("name", sc.MCTS)
def test_search_and_actor_match_reference(name):
    pc.check_mcts_golden("host", name, prefix=sc.MCTS_PREFIX)


def test_samples_of_finished_games_have_2k_plus_1_planes():
    assert pc.check_mcts_golden("host", "go5_p4_s48_k2", prefix=sc.MCTS_PREFIX)[1] == 3


@pytest.mark.parametrize("fmt", ["f32", "bf16", "f16", "f16_split"])
@pytest.mark.parametrize("name", ["go5_p4_s48_k2", "gomoku13_p8_s200_k1"])
def test_feature_layouts_match_reference(name, fmt):
    """2K+1 planes written in every feature layout decode to the reference's planes (the decoder checks that channels 2K+1..31 stay zero)."""
    pc.check_mcts_golden("host", name, sc.FEATS[fmt], prefix=sc.MCTS_PREFIX)


@pytest.mark.parametrize("k", [0, 9, -1])
def test_num_stack_out_of_range_is_rejected(k):
    from alpha_zero_amd.envs.go import GoEnv
    from alpha_zero_amd.envs.gomoku import GomokuEnv

    binding, dev = eu.backend("host")
    with pytest.raises(ValueError, match="1..8"):
        GoEnv(board_size=9, num_stack=k, _binding=binding, _device=dev)
    with pytest.raises(ValueError, match="1..8"):
        GomokuEnv(board_size=9, num_stack=k, _binding=binding, _device=dev)
    with pytest.raises(ValueError, match="1..8"):
        Engine(binding, EngineConfig(game="go", board_size=9, num_games=1, num_parallel=1, num_simulations=2, num_stack=k), device=dev)


def test_c_abi_num_stack_field():
    """AzspConfig.num_stack replaced a float with the same offset: 0 (a caller that predates the field) means 8, 9 is AZSP_EINVAL."""
    assert _abi.AzspConfig.num_stack.offset == _abi.AzspConfig.disable_resign_ratio.offset + 4 and _abi.AzspConfig.num_stack.size == 4
    b = eu.hosttwin_binding()
    for k, planes in ((0, 17), (8, 17), (1, 3), (4, 9), (9, None)):
        c = _abi.AzspConfig(game=_abi.GAME_GO, board_size=9, num_games=1, num_parallel=1, num_simulations=4, num_stack=k, seed=1)
        h = C.c_void_p()
        rc = b.dll.azsp_create(C.byref(c), C.byref(h))
        if planes is None:
            assert rc == -1 and not h.value
            continue
        assert rc == 0
        g = _abi.AzspGeometry()
        assert b.dll.azsp_geometry(h, C.byref(g)) == 0 and g.planes == planes
        b.dll.azsp_destroy(h)


def test_env_observation_and_copy_at_k2():
    """GoEnv(num_stack=2): 5-plane observations [X_t, Y_t, X_t-1, Y_t-1, C] rebuilt from the env's own K-deep board_deltas, and a deep
    copy (set_state with 2 history rows, padded to the engine's 8) observes the same planes."""
    import copy

    from alpha_zero_amd.envs.go import GoEnv

    binding, dev = eu.backend("host")
    env = GoEnv(board_size=9, num_stack=2, _binding=binding, _device=dev)
    rng = np.random.default_rng(3)
    for _ in range(7):
        legal = np.flatnonzero(env.legal_actions[:-1])
        obs, _, _, _ = env.step(int(rng.choice(legal)))
    assert obs.shape == (5, 9, 9) and len(env.board_deltas) == 2
    deltas = np.array(env.board_deltas)
    want = np.concatenate([np.stack([deltas == env.to_play, deltas == -env.to_play], 1).reshape(4, 9, 9),
                           np.full((1, 9, 9), env.to_play == 1)]).astype(np.int8)
    assert np.array_equal(obs, want)
    env2 = copy.deepcopy(env)
    assert env2.num_stack == 2 and np.array_equal(env2._eng.env_step(None, want_obs=True)["obs"][0], want)


def test_actor_refuses_a_network_of_another_input_depth():
    from alpha_zero_amd.core.network import AlphaZeroNet
    from alpha_zero_amd.core.pipeline import SelfPlayActor

    binding = eu.hosttwin_binding()
    kw = dict(game="go", board_size=5, num_games=2, num_simulations=4, num_parallel=2, device="cpu", net_dtype=torch.float32, use_graph=False,
              binding=binding)
    with pytest.raises(ValueError, match="9 input planes, but num_stack = 2 observations have 5"):
        SelfPlayActor(AlphaZeroNet((9, 5, 5), 26, 1, 8, 8), num_stack=2, **kw)
    with pytest.raises(ValueError, match="1..8"):
        SelfPlayActor(AlphaZeroNet((19, 5, 5), 26, 1, 8, 8), num_stack=9, **kw)
    a = SelfPlayActor(AlphaZeroNet((5, 5, 5), 26, 1, 8, 8), num_stack=2, **kw)
    with pytest.raises(ValueError, match="17 input planes"):
        a.set_network(AlphaZeroNet((17, 5, 5), 26, 1, 8, 8))


def test_uct_search_loads_a_k_row_history():
    """uct_search on an env with num_stack = 3 whose board_deltas holds 3 rows: the root observation eval_func receives is the env's."""
    from alpha_zero_amd.core.mcts_v2 import uct_search
    from alpha_zero_amd.envs.gomoku import GomokuEnv
    from synth_eval import make_eval_func

    binding, dev = eu.backend("host")
    env = GomokuEnv(board_size=9, num_stack=3, _binding=binding, _device=dev)
    for a in (40, 41, 31, 49, 22):
        env.step(a)
    seen = []
    inner = make_eval_func(env.action_dim)

    def eval_func(obs, batched=False):
        seen.append(np.array(obs))
        return inner(obs, batched)

    move, pi, _, _, _ = uct_search(env, eval_func, None, 19652.0, 1.25, num_simulations=16)
    assert seen[0].shape == (7, 9, 9) and np.array_equal(seen[0], env.observation())
    assert env.legal_actions[move] == 1 and abs(float(np.sum(pi)) - 1.0) < 1e-5


def test_sample_gather_two_ranks_gloo_k4(tmp_path):
    """2-rank gloo gather_samples of K = 4 samples ([n, 9, 5, 5]): every rank's samples arrive on rank 0 byte-identical."""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "stack_gather_worker.py")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29541")
    procs = [subprocess.Popen([sys.executable, script, str(r), "2", str(tmp_path)], env=env) for r in range(2)]
    assert all(p.wait(timeout=300) == 0 for p in procs)
    out = np.load(os.path.join(str(tmp_path), "rank0.npz"))
    games = out["games"]
    assert out["states"].shape[1:] == (9, 5, 5) and len(games) >= 2 and out["states"].shape[0] == games[:, _abi.GR_LENGTH].sum()
    assert set(np.unique(games[:, _abi.GR_SLOT] >> _abi.GR_SLOT_RANK_SHIFT)) == {0, 1}
    for r in range(2):
        eu.assert_rank_samples_gathered(out, r, np.load(os.path.join(str(tmp_path), f"local{r}.npz")))
