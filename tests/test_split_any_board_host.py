"""InferenceNet.use_split_any_board (opt-in, off by default): the path decision of the whole fp32-class evaluator on boards without a
tailored stem -- the wave-per-tile stem k_stem_spg in front of the wave-per-tile tower, azsp_head_split behind it.  Only the device type
is inspected, so the host twin's binding serves and no GPU is needed."""
import pytest
import torch

from alpha_zero_amd.core.network import AlphaZeroNet, InferenceNet

# fp32 x {64, 128, 256} x (Go 13, Go 19, Gomoku 13 at 128 / 256): the shapes whose tower runs k_conv3x3_spg behind a library stem and heads
_SHAPES = [(f, b, False) for f in (64, 128, 256) for b in (13, 19)] + [(f, 13, True) for f in (128, 256)]


def _net(filters, board, gomoku, planes=17):
    torch.manual_seed(0)
    return AlphaZeroNet((planes, board, board), board * board + (0 if gomoku else 1), 1, filters, 128, gomoku=gomoku)


def _answers(inf, board, device):
    return inf.evaluator_path(board, device), inf.supports_tiled_features(board, device), inf.supports_split_features(board, device)


@pytest.mark.parametrize("filters,board,gomoku", _SHAPES)
def test_split_any_board_path_decision_host_twin(filters, board, gomoku):
    import engine_util as eu

    inf = InferenceNet(_net(filters, board, gomoku), dtype=torch.float32, binding=eu.hosttwin_binding())
    assert inf.use_split_any_board is False
    off = {d: _answers(inf, board, d) for d in ("cuda", "cpu")}
    state_off = inf.capture_state()
    assert "behind a library fp32 stem and heads" in off["cuda"][0] and off["cuda"][1:] == (False, False)
    assert inf._path(board, "cuda") == ("split_tower", False, True)

    inf.use_split_any_board = True
    path, tiled, split = _answers(inf, board, "cuda")
    assert "hand-written" in path and "wave-per-tile" in path and "library" not in path, path
    assert (tiled, split) == (False, True)
    assert inf._path(board, "cuda") == ("split", False, True)
    assert _answers(inf, board, "cpu") == off["cpu"] and off["cpu"][0].startswith("library") and off["cpu"][1:] == (False, False)
    assert inf.capture_state() != state_off
    # the other switches keep their meaning: without the split heads or the split tower the answers are today's
    inf.use_split_heads = False
    assert _answers(inf, board, "cuda") == off["cuda"]
    inf.use_split_heads, inf.use_split_tower = True, False
    lib = _answers(inf, board, "cuda")
    assert lib[0].startswith("library") and lib[1:] == (False, False)
    inf.use_split_any_board = False
    assert _answers(inf, board, "cuda") == lib
    inf.use_split_tower = True
    assert _answers(inf, board, "cuda") == off["cuda"] and inf.capture_state() == state_off
    # a network whose fp32-class kernels were given up stays on the library
    inf.use_split_any_board, inf.split_fallback_reason = True, "the reason"
    assert inf.supports_split_features(board, "cuda") is False and inf.evaluator_path(board, "cuda").startswith("library fp32")
    # no binding: the library everywhere
    inf = InferenceNet(_net(filters, board, gomoku), dtype=torch.float32)
    inf.use_split_any_board = True
    got = _answers(inf, board, "cuda")
    assert got[0].startswith("library") and got[1:] == (False, False)


def test_split_any_board_leaves_other_networks_alone_host_twin():
    """A 40-plane stem (more than the stem kernels' 32 input channels), a bf16 network, the tailored shapes and a head too large for
    azsp_head_split's LDS answer the same with the switch on and off."""
    import engine_util as eu

    bnd = eu.hosttwin_binding()
    cases = [(InferenceNet(_net(128, 19, False, planes=40), dtype=torch.float32, binding=bnd), 19),
             (InferenceNet(_net(256, 19, False), dtype=torch.bfloat16, binding=bnd), 19),
             (InferenceNet(_net(64, 13, False), dtype=torch.bfloat16, binding=bnd), 13),
             (InferenceNet(_net(128, 9, False), dtype=torch.float32, binding=bnd), 9),
             (InferenceNet(_net(64, 13, True), dtype=torch.float32, binding=bnd), 13)]
    torch.manual_seed(0)
    wide = AlphaZeroNet((17, 19, 19), 362, 1, 64, 4096)  # 4 * (3 * 364 + 362 + 4096) * 4 B = 88 KB of LDS: beyond azsp_head_split
    cases.append((InferenceNet(wide, dtype=torch.float32, binding=bnd), 19))
    for inf, board in cases:
        off = [_answers(inf, board, d) for d in ("cuda", "cpu")] + [inf._path(board, "cuda")]
        inf.use_split_any_board = True
        assert [_answers(inf, board, d) for d in ("cuda", "cpu")] + [inf._path(board, "cuda")] == off, (inf.dtype, board)
    assert cases[0][0]._path(19, "cuda")[0] == "split_tower" and cases[-1][0]._path(19, "cuda")[0] == "split_tower"
    assert cases[3][0]._path(9, "cuda") == ("split", False, False)


def test_selfplay_actor_hands_the_switch_to_every_inference_net():
    """SelfPlayActor(split_any_board=...) sets use_split_any_board on the evaluator it builds first and on the one of set_network."""
    from alpha_zero_amd.core.pipeline import SelfPlayActor

    class _Stub(SelfPlayActor):  # (only the evaluator factory: no engine, no device)
        def __init__(self, on):
            import engine_util as eu

            self.net_dtype, self.binding, self.device = torch.float32, eu.hosttwin_binding(), torch.device("cuda")
            self.use_split_evaluator, self.split_any_board = True, on

    for on in (False, True):
        inf = _Stub(on)._inference_net(_net(64, 19, False))
        assert inf.use_split_any_board is on and inf.supports_split_features(19, "cuda") is on
