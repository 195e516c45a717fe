"""Device tier of the leaf symmetry (azsp_set_leaf_symmetry): the drivers of symmetry_checks.py on libazsp.so."""
import numpy as np
import pytest

import symmetry_checks as sc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("op", range(8))
@pytest.mark.parametrize("shape", ["go5", "go9", "gomoku7", "go19"])
def test_gpu_fixed_op_equals_the_plain_search_around_the_wrapped_evaluator(shape, op):
    sc.check_fixed_op("gpu", shape, op)


def test_gpu_fixed_op_in_the_remaining_feature_layouts():
    sc.check_fixed_op("gpu", "go5", 3, dtypes=sc.OTHER_DTYPES)


@pytest.mark.parametrize("shape,dtype", [("go5", sc._abi.FEAT_I8), ("go9", sc._abi.FEAT_BF16_TILED), ("gomoku7", sc._abi.FEAT_F16_SPLIT)])
def test_gpu_random_mode_equals_the_plain_search_when_the_evaluator_undoes_each_rows_op(shape, dtype):
    sc.check_random_mode("gpu", shape, dtype)


def test_gpu_random_ops_are_the_recomputed_draws_and_those_of_the_host_twin():
    sc.check_stream("gpu")
    dev, host = sc.stream_ops("gpu")[0], sc.stream_ops("host")[0]
    assert len(dev) == len(host) and all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(dev, host))


def test_gpu_op_0_and_a_mode_turned_off_are_the_plain_engine():
    sc.check_identity_and_off("gpu")


def test_gpu_op_0_is_the_plain_resident_search_behind_a_device_evaluator():
    sc.check_resident_identity_gpu()


@pytest.mark.parametrize("game,n,P", [("go", 5, 1), ("go", 5, 4), ("gomoku", 7, 1)])
def test_gpu_batch_search_with_a_host_eval_func(game, n, P):
    sc.check_batch_search("gpu", game, n, P)


def test_gpu_actor_with_random_symmetry_harvests_true_orientation_games():
    sc.check_actor_random("gpu")


def test_gpu_bad_modes_are_refused():
    sc.check_refusals("gpu")
