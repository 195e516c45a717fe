"""Exact-operand tier on the host twin (tests/exact_checks.py): the generators, preconditions and references are proven against the
plain-loop restatement of every evaluator entry point before a device is involved.  Operands exact, comparison bitwise, preconditions
asserted.  Shapes: C = 16, S = 5 for the tiled family (the f16 convolution and stem at the one shape the twin restates, 9x9 x 128), the
tailored shapes for the fp32-class family."""
import pytest
import torch

import engine_util as eu
import exact_checks as ec

FMTS = {"bf16": ec.BF16, "f16": ec.F16}


def _twin():
    return eu.hosttwin_binding()


# ---------------------------------------------------------------------------------------------------
# the tier's own tools
# ---------------------------------------------------------------------------------------------------
def test_quantum_and_exact_sum_rule():
    assert ec.quantum(torch.tensor([3.0, 0.0, 8.0])) == 1.0
    assert ec.quantum(torch.tensor([5.0 + 3 / 2048, 6.0])) == 1 / 2048
    assert ec.quantum(torch.tensor([0.375, -12.0])) == 0.125
    assert ec.quantum(torch.zeros(3)) == float("inf")
    ec.assert_sums_exact(torch.tensor([2.0 ** 20 - 1]), 1.0, 20, "fits")
    with pytest.raises(AssertionError, match="generator is wrong"):
        ec.assert_sums_exact(torch.tensor([2.0 ** 20]), 1.0, 20, "does not fit")
    with pytest.raises(AssertionError, match="generator is wrong"):
        ec.assert_sums_exact(torch.tensor([2.0 ** 10]), 2.0 ** -14, 24, "does not fit")


def test_rounding_shares_count_inexact_values_and_ties():
    # bf16 keeps 8 bits: 257 and 259 are ties between 256 / 258 / 260, 513 rounds but is no tie (neighbours 512, 516), 258 is exact
    ref = torch.tensor([257.0, 259.0, 513.0, 258.0, 0.0, -257.0, 3.0, 1.0], dtype=torch.float64)
    assert ec.rounding_shares(ref, ec.BF16) == (4 / 8, 3 / 8)
    # f16 keeps 11 bits: 2049 is a tie, 4097 is not, 2050 is exact
    assert ec.rounding_shares(torch.tensor([2049.0, 4097.0, 2050.0, 5.0], dtype=torch.float64), ec.F16) == (2 / 4, 1 / 4)
    # and torch's conversion, the expected value of the tier, rounds ties to even
    assert torch.tensor([257.0, 259.0]).to(torch.bfloat16).tolist() == [256.0, 260.0]
    assert torch.tensor([2049.0, 2051.0]).to(torch.float16).tolist() == [2048.0, 2052.0]


def test_failure_message_names_the_cells():
    a = torch.zeros(2, 8, 5, 5)
    b = a.clone()
    b[1, 3, 4, 0] = 2.0
    with pytest.raises(AssertionError, match=r"1 of 400 cells differ.*\(1, 3, 4, 0\), 0.0, 2.0.*per row \[0, 0, 0, 0, 1\].*per column \[1, 0, 0, 0, 0\]"):
        ec.assert_same_cells(a, b, "demo")


def test_batches_are_built_from_patterns():
    idx = ec.pattern_index(770)
    assert idx[:5].tolist() == [0, 7, 14, 21, 4] and sorted(set(idx.tolist())) == list(range(ec.PATTERNS))


# ---------------------------------------------------------------------------------------------------
# bf16 / f16 evaluator
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [0, 1])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("boards", [1, 4])
def test_tiled_conv_exact_host_twin(boards, relu, res):
    ec.tiled_conv_exact(_twin(), "cpu", 5, 16, boards, ec.BF16, res, relu)


@pytest.mark.parametrize("res,relu", [(1, 1), (0, 0)])
def test_tiled_conv_f16_exact_host_twin(res, relu):
    ec.tiled_conv_exact(_twin(), "cpu", 9, 128, 1, ec.F16, res, relu)


@pytest.mark.parametrize("boards", [1, 4])
def test_tiled_resblock_exact_host_twin(boards):
    ec.tiled_resblock_exact(_twin(), "cpu", 5, 16, boards)


@pytest.mark.parametrize("pad,boards,relu", [(1, 1, 1), (1, 4, 0), (3, 3, 1)])
def test_tiled_stem_exact_host_twin(pad, boards, relu):
    ec.tiled_stem_exact(_twin(), "cpu", 5, 16, pad, boards, ec.BF16, relu=relu)


def test_tiled_stem_f16_exact_host_twin():
    ec.tiled_stem_exact(_twin(), "cpu", 9, 128, 1, 1, ec.F16)


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("strided", [False, True])
def test_tiled_head_exact_host_twin(strided, fmt):
    ec.tiled_head_exact(_twin(), "cpu", 5, 16, 4, FMTS[fmt], strided)


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_fc_heads_exact_host_twin(fmt):
    ec.fc_heads_exact(_twin(), "cpu", 25, 26, 16, 5, FMTS[fmt])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("channels", [8, 64, 128, 256])
def test_bias_act_exact_host_twin(channels, dtype):
    for rows in (1, 37 * 81):
        for res in (0, 1):
            for relu in (0, 1):
                ec.bias_act_exact(_twin(), "cpu", rows, channels, dtype, res, relu)


# ---------------------------------------------------------------------------------------------------
# fp32-class evaluator
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ints", "carry"])
@pytest.mark.parametrize("S,C,boards", [(9, 128, 3), (9, 64, 2), (17, 64, 2), (5, 64, 3)])
def test_split_conv_exact_host_twin(S, C, boards, kind):
    for res, relu in ((1, 1), (0, 0), (1, 0), (0, 1)):
        ec.split_conv_exact(_twin(), "cpu", S, C, boards, kind, res, relu)


@pytest.mark.parametrize("kind", ["ints", "carry"])
@pytest.mark.parametrize("S,boards", [(17, 2), (9, 3)])
def test_split_resblock_exact_host_twin(S, boards, kind):
    ec.split_resblock_exact(_twin(), "cpu", S, boards, kind)


@pytest.mark.parametrize("kind", ["carry", "exact"])
@pytest.mark.parametrize("n,C,pad", [(9, 128, 1), (9, 64, 1), (13, 64, 3)])
def test_split_stem_exact_host_twin(n, C, pad, kind):
    ec.split_stem_exact(_twin(), "cpu", n, C, pad, 2, kind)
    ec.split_stem_exact(_twin(), "cpu", n, C, pad, 1, kind, relu=0)


@pytest.mark.parametrize("S,C,A,Fw", [(9, 128, 82, 128), (9, 64, 82, 64), (17, 64, 169, 64)])
def test_head_split_exact_host_twin(S, C, A, Fw):
    ec.head_split_exact(_twin(), "cpu", S, C, A, Fw, 3)


def test_carry_needs_five_to_seven():
    """Why the carry values start at 5: 4 - 3 / 2048 rounds to an f16 that is no integer (half a step below 4 is 2 / 2048), and a hi plane of
    non-integers makes the hi x hi products longer than fp32's 24 bits."""
    hi, lo = ec.split_parts(torch.tensor([4 - 3 / 2048, 5 - 3 / 2048, 7 + 3 / 2048], dtype=torch.float64))
    assert hi[0] != hi[0].round() and hi[1:].tolist() == [5.0, 7.0] and lo[1:].tolist() == [-3.0, 3.0]
