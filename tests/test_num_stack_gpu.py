"""GPU tier of the observation history depth num_stack = K (1..8, 2K+1 planes) on libazsp.so: the reference's playouts and search /
actor goldens at K < 8, every feature layout against the plain planes, a 2K+1-input network on the fp32-class split path, the
batched actor and the drop-in search at K < 8."""
import numpy as np
import pytest
import torch

import engine_util as eu
import golden_mcts
import parity_checks as pc
import stack_checks as sc
from alpha_zero_amd import _abi
from synth_eval import eval_batch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("game,n,k", sc.PLAYOUTS)
def test_gpu_playouts_match_reference(game, n, k):
    sc.check_playouts("gpu", game, n, k)


@pytest.mark.parametrize("fmt", ["i8", "f16_split", "bf16"])
@pytest.mark.parametrize("name", sc.MCTS)
def test_gpu_search_and_actor_match_reference(name, fmt):
    pc.check_mcts_golden("gpu", name, sc.FEATS[fmt], prefix=sc.MCTS_PREFIX)


@pytest.mark.parametrize("k", [1, 4, 8])
def test_gpu_every_feature_layout_is_the_plain_planes(k):
    """One position set (the first rounds of the go5 golden's games) written under every feature_dtype decodes to the I8 planes; at
    K = 8 the tiled / split tensors are byte for byte the 17-plane encodings (engine_util.tile_features / split_features)."""
    G = golden_mcts.MctsGolden("go5_p4_s48_k2", sc.MCTS_PREFIX)
    got = {}
    raw = {}
    for fmt, fd in sc.FEATS.items():
        seen = []

        def keep(r, feats, eng, seen=seen, fmt=fmt):
            if r < 40:
                seen.append(feats.copy())
                if r == 20:
                    raw[fmt] = eng.features.clone().cpu()

        eu.run_golden_selfplay("gpu", G, eval_batch, fd, num_stack=k, on_features=keep, max_rounds=40)
        got[fmt] = np.stack(seen)
    assert got["i8"].shape[2] == 2 * k + 1
    for fmt in sc.FEATS:
        assert np.array_equal(got[fmt], got["i8"]), fmt
    if k == 8:
        x = torch.from_numpy(got["i8"][20]).float()
        for fmt, want in (("bf16", eu.tile_features(x, torch.bfloat16)), ("f16", eu.tile_features(x, torch.float16)), ("f16_split", eu.split_features(x))):
            have, want = raw[fmt].view(torch.int16), want.view(torch.int16)
            m = min(have.numel(), want.numel())
            assert torch.equal(have[:m], want[:m]) and not have[m:].any() and not want[m:].any(), fmt


@pytest.mark.parametrize("game,n,filters", [("go", 9, 128), ("gomoku", 13, 64)])
def test_gpu_split_evaluator_on_engine_features_k4(game, n, filters):
    """A 9-input network (K = 4) on the fp32-class split path, fed the engine's own AZSP_FEAT_F16_SPLIT features, vs the fp64 module
    (tests/test_split_tower.py's bounds: 2e-6 on priors and values)."""
    from alpha_zero_amd.core.engine import Engine, EngineConfig
    from alpha_zero_amd.core.network import AlphaZeroNet, InferenceNet

    torch.manual_seed(0)
    A = n * n + (1 if game == "go" else 0)
    net = AlphaZeroNet((9, n, n), A, 2, filters, 64, gomoku=game == "gomoku").eval()
    b = eu.gpu_binding()
    inf = InferenceNet(net, dtype=torch.float32, binding=b).cuda()
    assert inf.supports_split_features(n, "cuda")
    eng = Engine(b, EngineConfig(game=game, board_size=n, num_games=8, num_parallel=4, num_simulations=16, num_stack=4,
                                 feature_dtype=_abi.FEAT_F16_SPLIT, seed=5), device="cuda")
    eng.reset_games()
    eng.select()
    rng = np.random.default_rng(1)
    for _ in range(30):  # a few rounds with random priors: leaves with non-empty histories
        eng.priors.copy_(torch.from_numpy(rng.dirichlet(np.ones(A), eng.rows).astype(np.float32)))
        eng.values.copy_(torch.from_numpy(rng.uniform(-0.5, 0.5, eng.rows).astype(np.float32)))
        eng.round()
    planes = eu.decode_features(eng)
    assert planes.shape == (eng.rows, 9, n, n) and planes[:, :8].any()
    pri = torch.zeros(eng.rows, A, device="cuda")
    val = torch.zeros(eng.rows, device="cuda")
    inf.forward_split(eng.features, pri, val, split_features=(eng.rows, n))
    with torch.no_grad():
        lg, v64 = net.double()(torch.from_numpy(planes).double())
    dp = (pri.cpu().double() - torch.softmax(lg, -1)).abs().max().item()
    dv = (val.cpu().double() - v64.squeeze(1)).abs().max().item()
    assert dp <= 2e-6 and dv <= 2e-6, (dp, dv)
    eng.close()


def test_gpu_actor_k4_harvest_replays_on_the_host_twin():
    """SelfPlayActor at K = 4 (9x9, G = 256): harvested states are [n, 9, 9, 9] and equal the observations of a host-twin env replaying
    the harvested moves."""
    from alpha_zero_amd.core.network import AlphaZeroNet
    from alpha_zero_amd.core.pipeline import SelfPlayActor
    from alpha_zero_amd.envs.go import GoEnv

    torch.manual_seed(0)
    net = AlphaZeroNet((9, 9, 9), 82, 1, 64, 64)
    a = SelfPlayActor(net, game="go", board_size=9, num_games=256, num_simulations=16, num_parallel=4, warm_up_steps=4, seed=3, num_stack=4)
    out = []
    for _ in range(80):
        a.run_rounds(25)
        out += a.harvest(with_moves=True)
        if len(out) >= 3:
            break
    assert out, "no game finished"
    hb, hd = eu.backend("host")
    for seq, stats, moves in out[:3]:
        env = GoEnv(board_size=9, num_stack=4, _binding=hb, _device=hd)
        assert seq[0].state.shape == (9, 9, 9)
        for t, tr in enumerate(seq):
            assert np.array_equal(tr.state, env.observation()), t
            if t < len(moves):
                env.step(moves[t])


def test_gpu_uct_search_with_device_evaluator_k1():
    """uct_search at K = 1 with a DeviceEvaluator (3-input network): the device-resident loop and the host-callback loop with the same
    evaluator pick the same move with the same pi; a network of the wrong depth is refused before the search."""
    from alpha_zero_amd.core.evaluate import DeviceEvaluator
    from alpha_zero_amd.core.mcts_v2 import uct_search
    from alpha_zero_amd.core.network import AlphaZeroNet, InferenceNet
    from alpha_zero_amd.envs.go import GoEnv

    torch.manual_seed(0)
    b = eu.gpu_binding()
    net = AlphaZeroNet((3, 9, 9), 82, 1, 64, 64).eval()
    ev = DeviceEvaluator(InferenceNet(net, dtype=torch.float32, binding=b).cuda(), use_graph=False)
    assert ev.in_channels == 3
    env = GoEnv(board_size=9, num_stack=1)
    for a in (40, 30, 50):
        env.step(a)
    r_dev = uct_search(env, ev, None, 19652.0, 1.25, num_simulations=48, deterministic=True)
    r_cb = uct_search(env, lambda o, batched=False: ev(o, batched), None, 19652.0, 1.25, num_simulations=48, deterministic=True)
    assert r_dev[0] == r_cb[0] and np.array_equal(r_dev[1], r_cb[1]) and env.legal_actions[r_dev[0]] == 1
    ev17 = DeviceEvaluator(InferenceNet(AlphaZeroNet((17, 9, 9), 82, 1, 64, 64).eval(), dtype=torch.float32, binding=b).cuda(), use_graph=False)
    with pytest.raises(ValueError, match="17 input planes"):
        uct_search(env, ev17, None, 19652.0, 1.25, num_simulations=8)
