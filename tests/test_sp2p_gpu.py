"""k_conv3x3_sp2p (alpha_zero_amd/csrc/az_conv_sp2p.h): the 9x9 x 128 fp32-class convolution over PAIRS of boards, without the MFMAs that only
multiply the zero padding of the edge tiles.  A skipped MFMA would add exact zeros, so it must agree word for word with the
wave-per-tile kernel (k_conv3x3_spg, HALVES = 2: the same two accumulation chains), which takes no part in the pair scheme and multiplies the padding; and it must keep the fp64 bound of
tests/test_split_tower.py.  Board counts follow the persistent loop's paths on the device at hand (slots = CUs / 2 pairs in flight)."""
import functools

import pytest
import torch

import split_util as su

C, S = 128, 9
CASES = ((False, 1), (False, 0), (True, 1), (True, 0))  # (residual, relu)
COUNTS = ("one_pair", "pair_and_odd_tail", "one_pair_per_slot", "some_slots_with_a_second_pair", "six_and_seven_pairs_per_slot_and_odd_tail")


def _boards(name):
    """256-CU device: 2, 3, 256, 258, 1617 (slots with 6 and 7 pairs = a full 12-board corner batch, and a full batch + a partial one)."""
    slots = max(1, torch.cuda.get_device_properties(0).multi_processor_count // 2)
    return {COUNTS[0]: 2, COUNTS[1]: 3, COUNTS[2]: 2 * slots, COUNTS[3]: 2 * slots + 2, COUNTS[4]: 2 * (6 * slots + 5 * slots // 16) + 1}[name]


@functools.lru_cache(maxsize=None)
def _inputs(boards):
    """x, r, w, b and the fp64 convolution + bias of x (computed once per board count, never modified)."""
    x, r, w, b = su.conv_inputs(boards, C, S, 700 + boards)
    x = x - 0.3  # both signs, so that the cases without ReLU carry negative outputs
    return x, r, w, b, su.ref64_conv(x, None, w, b, 0)


def _conv(bnd, boards, res, relu, waves):
    x, r, w, b, _ = _inputs(boards)
    with su.small_batch_waves(bnd.dll, waves):
        return su.split_conv(bnd, x, r if res else None, w, b, relu, "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("count", COUNTS)
def test_gpu_pair_kernel_is_bit_identical_to_the_wave_per_tile_kernel(count):
    from alpha_zero_amd import _lib

    bnd = _lib.load()
    boards = _boards(count)
    for res, relu in CASES:
        a = _conv(bnd, boards, res, relu, 0)         # tailored path: k_conv3x3_sp2p on the pairs, a one-board k_conv3x3_spg launch on an odd last board
        g = _conv(bnd, boards, res, relu, 1 << 20)   # k_conv3x3_spg on the whole call
        su.assert_same_words(a.raw, g.raw, boards, C, S, f"boards={boards} res={res} relu={relu}", a.y, g.y)
    # res == y (include/azsp.h allows it): a wave loads the residual of its own elements before it stores them
    x, r, w, b, _ = _inputs(boards)
    dll = bnd.dll
    xs, ys = su.to_split(dll, x, "cuda"), su.to_split(dll, r, "cuda")
    wsp, bb = su.split_params(w, b, "cuda")
    with su.small_batch_waves(dll, 0):
        assert dll.azsp_conv3x3_split(xs.data_ptr(), wsp.data_ptr(), bb.data_ptr(), ys.data_ptr(), ys.data_ptr(), boards, S, C, 1, None, None) == 0
    torch.cuda.synchronize()
    su.assert_same_words(ys.cpu(), _conv(bnd, boards, True, 1, 1 << 20).raw, boards, C, S, f"boards={boards} res == y")


@pytest.mark.gpu
@pytest.mark.parametrize("count", COUNTS)
def test_gpu_pair_kernel_error_vs_fp64(count):
    """The absolute bound of tests/test_split_tower.py::test_gpu_split_conv_error_vs_fp64: <= 8e-7 of max |y64|."""
    from alpha_zero_amd import _lib

    bnd = _lib.load()
    boards = _boards(count)
    _, r, _, _, pre = _inputs(boards)
    for res, relu in CASES:
        ref = pre + r.double() if res else pre
        ref = torch.relu(ref) if relu else ref
        o = _conv(bnd, boards, res, relu, 0)
        err = su.rel_err(o.y, ref)
        print(f"boards={boards} res={res} relu={relu} err={err:.3g} roundtrip={o.roundtrip:.3g}")
        assert o.roundtrip <= 2.0 ** -21 and err <= 8e-7, (boards, res, relu, err, o.roundtrip)
