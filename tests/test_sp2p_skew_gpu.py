"""k_conv3x3_sp2p's skewed units (alpha_zero_amd/csrc/az_conv_sp2p.h): U0 and U3 read ONE B fragment per step for all their tiles and walk
the taps in a skewed order.  No output bit may move: the words must equal the wave-per-tile kernel's (k_conv3x3_spg, HALVES = 2: the same
accumulation chains, a fragment per tile, none of the pair kernel's memory scheme) with the residual ALIASED to y -- a lane must have loaded
every cell's residual, the corner cells' included, before a store of the call can touch it -- at
  2 (6 slots + 5 slots // 16) + 1 boards   every slot runs six or seven pairs of the steady-state loop: a full corner batch of 12 boards,
                                           then (in 5 of 16 slots) a partial batch of 2; the odd last board runs the wave-per-tile kernel;
  26 boards                                13 slots with one pair each: corner batches of 2 boards on a slot's first and last pair.
(The board counts are those at which a corner batch's residual, if loaded a unit before the corner phase, would meet every batch shape: that
placement was measured and left out; the cases hold for any placement.)"""
import functools

import pytest
import torch

import split_util as su

C, S = 128, 9


def _slots():
    return max(1, torch.cuda.get_device_properties(0).multi_processor_count // 2)


@functools.lru_cache(maxsize=None)
def _inputs(boards):
    x, r, w, b = su.conv_inputs(boards, C, S, 4100 + boards % 1000)
    return x - 0.3, r, w, b  # both signs: the cases without ReLU carry negative outputs


@functools.lru_cache(maxsize=None)
def _wave_per_tile(boards, relu):
    """the reference words: k_conv3x3_spg on the whole call (computed once per case, never modified)"""
    from alpha_zero_amd import _lib

    bnd = _lib.load()
    x, r, w, b = _inputs(boards)
    with su.small_batch_waves(bnd.dll, 1 << 20):
        return su.split_conv(bnd, x, r, w, b, relu, "cuda").raw


def _pair_kernel_aliased(boards, relu):
    from alpha_zero_amd import _lib

    dll = _lib.load().dll
    x, r, w, b = _inputs(boards)
    xs, ys = su.to_split(dll, x, "cuda"), su.to_split(dll, r, "cuda")  # y holds the residual
    wsp, bb = su.split_params(w, b, "cuda")
    with su.small_batch_waves(dll, 0):
        assert dll.azsp_conv3x3_split(xs.data_ptr(), wsp.data_ptr(), bb.data_ptr(), ys.data_ptr(), ys.data_ptr(), boards, S, C, relu, None, None) == 0
    torch.cuda.synchronize()
    return ys.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("relu", (0, 1))
@pytest.mark.parametrize("case", ("full_then_partial_batch", "batches_of_two"))
def test_gpu_skewed_pair_kernel_words_with_the_residual_aliased_to_y(case, relu):
    slots = _slots()
    boards = 2 * (6 * slots + 5 * slots // 16) + 1 if case == "full_then_partial_batch" else 26
    su.assert_same_words(_pair_kernel_aliased(boards, relu), _wave_per_tile(boards, relu), boards, C, S, f"{case}: boards={boards} res == y relu={relu}")
