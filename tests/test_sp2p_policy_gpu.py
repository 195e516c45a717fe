"""k_conv3x3_sp2p's memory side (alpha_zero_amd/csrc/az_conv_sp2p.h): which tile a position's output leaves in (the pair table) and the cache
policy of its residual loads, image pieces and stores may change, no output bit may.  The words must equal the wave-per-tile kernel's
(k_conv3x3_spg, HALVES = 2: the same accumulation chains, none of the pair kernel's memory scheme) with the residual absent, in a buffer
of its own, and aliased to y (include/azsp.h allows res == y: a lane loads the residual of its own elements before it stores them), at
  2 boards       one pair: every unit is the first and the last of its slot at once, the corner batch holds 2 boards;
  26 boards      13 slots with one pair each: the other paths of a short call, corner batches of n_ok = 2 < 12 boards whose residual is
                 loaded in the corner phase;
  2 slots + 2    one slot runs a second pair: the steady-state loop, the only path on which the prefetch of the next pair's image
                 (issued while the previous pair's stores are in flight) is live -- checked with the residual aliased to y."""
import functools

import pytest
import torch

import split_util as su

C, S = 128, 9


@functools.lru_cache(maxsize=None)
def _inputs(boards):
    x, r, w, b = su.conv_inputs(boards, C, S, 900 + boards)
    return x - 0.3, r, w, b  # both signs: the cases without ReLU carry negative outputs


@functools.lru_cache(maxsize=None)
def _wave_per_tile(boards, res, relu):
    """the reference words: k_conv3x3_spg on the whole call (computed once per case, never modified)"""
    from alpha_zero_amd import _lib

    bnd = _lib.load()
    x, r, w, b = _inputs(boards)
    with su.small_batch_waves(bnd.dll, 1 << 20):
        return su.split_conv(bnd, x, r if res else None, w, b, relu, "cuda").raw


def _pair_kernel(boards, res, relu):
    """res: None, "separate" or "aliased" (y is the buffer that holds the residual)"""
    from alpha_zero_amd import _lib

    dll = _lib.load().dll
    x, r, w, b = _inputs(boards)
    xs, rs = su.to_split(dll, x, "cuda"), su.to_split(dll, r, "cuda")
    ys = rs if res == "aliased" else torch.zeros_like(xs)
    wsp, bb = su.split_params(w, b, "cuda")
    with su.small_batch_waves(dll, 0):
        assert dll.azsp_conv3x3_split(xs.data_ptr(), wsp.data_ptr(), bb.data_ptr(), rs.data_ptr() if res else None, ys.data_ptr(), boards, S, C, relu, None, None) == 0
    torch.cuda.synchronize()
    return ys.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("boards", (2, 26))
@pytest.mark.parametrize("relu", (0, 1))
@pytest.mark.parametrize("res", (None, "separate", "aliased"))
def test_gpu_pair_kernel_words_with_every_residual_placement(boards, relu, res):
    su.assert_same_words(_pair_kernel(boards, res, relu), _wave_per_tile(boards, res is not None, relu), boards, C, S, f"boards={boards} res={res} relu={relu}")


@pytest.mark.gpu
def test_gpu_pair_kernel_aliased_residual_in_the_steady_state_loop():
    slots = max(1, torch.cuda.get_device_properties(0).multi_processor_count // 2)
    boards = 2 * slots + 2
    su.assert_same_words(_pair_kernel(boards, "aliased", 1), _wave_per_tile(boards, True, 1), boards, C, S, f"boards={boards} res == y")
