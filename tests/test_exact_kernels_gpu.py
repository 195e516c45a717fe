"""Exact-operand tier on the device (tests/exact_checks.py): every evaluator entry point of include/azsp.h bit for bit against fp64.
Operands exact, comparison bitwise, preconditions asserted -- no tolerance anywhere except after exp / tanh in the heads, where the bounds
are derived (exact_checks.PRIOR_REL, VALUE_ABS, SUM_ABS).  Board counts are the smallest that reach each path of a kernel: one board, a
ragged last tile or pair, more than one workgroup, and beyond one pass of the persistent workgroups."""
import pytest
import torch

import exact_checks as ec
import split_util as su

FMTS = {"bf16": ec.BF16, "f16": ec.F16}
ALL4 = ((1, 1), (0, 0), (1, 0), (0, 1))  # (residual, relu)


def _lib():
    from alpha_zero_amd import _lib

    return _lib.load()


def _cases(table):
    return [(*shape, b) for shape, boards in table for b in boards]


# ---------------------------------------------------------------------------------------------------
# bf16 / f16 evaluator
# ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("S,C,boards", _cases([((9, 128), (1, 2, 7, 770)), ((9, 64), (1, 4, 770)), ((17, 64), (1, 2, 257)), ((19, 256), (1, 2, 33))]))
def test_gpu_tiled_conv_exact(S, C, boards):
    for res, relu in ALL4:
        ec.tiled_conv_exact(_lib(), "cuda", S, C, boards, ec.BF16, res, relu)


@pytest.mark.gpu
@pytest.mark.parametrize("boards", [1, 7, 770])
def test_gpu_tiled_conv_f16_exact(boards):
    for res, relu in ALL4:
        ec.tiled_conv_exact(_lib(), "cuda", 9, 128, boards, ec.F16, res, relu)


@pytest.mark.gpu
@pytest.mark.parametrize("S,boards", _cases([((17,), (1, 2, 257)), ((9,), (1, 4, 770))]))
def test_gpu_tiled_resblock_exact(S, boards):
    ec.tiled_resblock_exact(_lib(), "cuda", S, 64, boards)


@pytest.mark.gpu
@pytest.mark.parametrize("boards", [1, 5])
@pytest.mark.parametrize("n,C,pad,fmt", [(9, 128, 1, "bf16"), (9, 64, 1, "bf16"), (13, 64, 3, "bf16"), (19, 256, 1, "bf16"), (9, 128, 1, "f16")])
def test_gpu_tiled_stem_exact(n, C, pad, fmt, boards):
    ec.tiled_stem_exact(_lib(), "cuda", n, C, pad, boards, FMTS[fmt])
    ec.tiled_stem_exact(_lib(), "cuda", n, C, pad, boards, FMTS[fmt], relu=0)


@pytest.mark.gpu
@pytest.mark.parametrize("boards", [1, 5])
@pytest.mark.parametrize("C,S,fmt", [(128, 9, "bf16"), (64, 17, "bf16"), (256, 19, "bf16"), (128, 9, "f16")])
def test_gpu_tiled_head_exact(C, S, fmt, boards):
    for strided in (False, True):
        ec.tiled_head_exact(_lib(), "cuda", S, C, boards, FMTS[fmt], strided)


@pytest.mark.gpu
@pytest.mark.parametrize("boards", [1, 33, 130])
@pytest.mark.parametrize("P2,A,Fw,fmt", [(81, 82, 128, "bf16"), (81, 82, 64, "bf16"), (289, 169, 64, "bf16"), (81, 82, 128, "f16")])
def test_gpu_fc_heads_exact(P2, A, Fw, fmt, boards):
    ec.fc_heads_exact(_lib(), "cuda", P2, A, Fw, boards, FMTS[fmt])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("channels", [8, 64, 128, 256])
def test_gpu_bias_act_exact(channels, dtype):
    for rows in (1, 37 * 81):
        for res, relu in ALL4:
            ec.bias_act_exact(_lib(), "cuda", rows, channels, dtype, res, relu)


# ---------------------------------------------------------------------------------------------------
# fp32-class evaluator
# ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ints", "carry"])
@pytest.mark.parametrize("S,C,boards", _cases([((9, 128), (1, 2, 3, 257, 515)), ((9, 64), (1, 2, 3, 257, 515)), ((17, 64), (1, 2, 3, 257, 515))]))
def test_gpu_split_conv_exact(S, C, boards, kind):
    """The weight-stationary kernels at every board count (limit 0: an odd last board of (9, 128) still runs the wave-per-tile kernel), and
    whatever the default limit picks."""
    bnd = _lib()
    with su.small_batch_waves(bnd.dll, 0):
        for res, relu in ALL4[:2] if boards > 3 else ALL4:
            ec.split_conv_exact(bnd, "cuda", S, C, boards, kind, res, relu)
    for res, relu in ALL4:
        ec.split_conv_exact(bnd, "cuda", S, C, boards, kind, res, relu)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ints", "carry"])
@pytest.mark.parametrize("S,C,boards", [(19, 256, 2), (13, 64, 4), (5, 64, 7), (25, 64, 2)])
def test_gpu_split_conv_wave_per_tile_exact(S, C, boards, kind):
    """Shapes without a tailored kernel: k_conv3x3_spg, and under a limit of one wave the 48-position kernel k_conv3x3_spgw."""
    bnd = _lib()
    for res, relu in ALL4:
        ec.split_conv_exact(bnd, "cuda", S, C, boards, kind, res, relu)
    with su.small_batch_waves(bnd.dll, 1):
        for res, relu in ALL4:
            ec.split_conv_exact(bnd, "cuda", S, C, boards, kind, res, relu)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ints", "carry"])
@pytest.mark.parametrize("S,boards", _cases([((17,), (1, 2, 257, 513)), ((9,), (1, 2, 3, 513, 514))]))
def test_gpu_split_resblock_exact(S, boards, kind):
    bnd = _lib()
    with su.small_batch_waves(bnd.dll, 0):
        ec.split_resblock_exact(bnd, "cuda", S, boards, kind)
    ec.split_resblock_exact(bnd, "cuda", S, boards, kind)


_STEMS = _cases([((9, 128, 1), (1, 5, 203)), ((9, 64, 1), (1, 5, 203)), ((13, 64, 3), (1, 5, 203)), ((19, 64, 1), (2,)), ((15, 64, 3), (2,))])


@pytest.mark.gpu
@pytest.mark.parametrize("n,C,pad,boards", _STEMS)
def test_gpu_split_features_and_stem_exact(n, C, pad, boards):
    """azsp_split_features + azsp_stem_split on carry planes, 17 of the 32 channels."""
    ec.split_stem_exact(_lib(), "cuda", n, C, pad, boards, "carry")
    if boards <= 2:
        ec.split_stem_exact(_lib(), "cuda", n, C, pad, boards, "carry", relu=0)


@pytest.mark.gpu
@pytest.mark.parametrize("n,C,pad,boards", _STEMS)
def test_gpu_stem_split_exact_exact(n, C, pad, boards):
    """azsp_stem_split_exact on 0 / 1 planes: exact, and word for word azsp_stem_split."""
    ec.split_stem_exact(_lib(), "cuda", n, C, pad, boards, "exact")


@pytest.mark.gpu
@pytest.mark.parametrize("boards", [1, 3, 4, 5, 9])
@pytest.mark.parametrize("S,C,A,Fw", [(9, 128, 82, 128), (9, 64, 82, 64), (17, 64, 169, 64)])
def test_gpu_head_split_exact(S, C, A, Fw, boards):
    ec.head_split_exact(_lib(), "cuda", S, C, A, Fw, boards)
