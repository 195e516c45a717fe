"""CPU tier of the leaf symmetry (azsp_set_leaf_symmetry): the drivers of symmetry_checks.py on the host twin."""
import pytest

import symmetry_checks as sc


def test_numpy_transforms_are_the_documented_index_maps():
    sc.check_transforms_are_the_documented_maps()


@pytest.mark.parametrize("op", range(8))
@pytest.mark.parametrize("shape", ["go5", "go9", "gomoku7", "go19"])
def test_fixed_op_equals_the_plain_search_around_the_wrapped_evaluator(shape, op):
    sc.check_fixed_op("host", shape, op)


def test_fixed_op_in_the_remaining_feature_layouts():
    sc.check_fixed_op("host", "go5", 3, dtypes=sc.OTHER_DTYPES)


@pytest.mark.parametrize("shape,dtype", [("go5", sc._abi.FEAT_I8), ("go9", sc._abi.FEAT_BF16_TILED), ("gomoku7", sc._abi.FEAT_F16_SPLIT)])
def test_random_mode_equals_the_plain_search_when_the_evaluator_undoes_each_rows_op(shape, dtype):
    sc.check_random_mode("host", shape, dtype)


def test_random_ops_are_the_recomputed_draws_of_a_stream_of_their_own():
    sc.check_stream("host")


def test_op_0_and_a_mode_turned_off_are_the_plain_engine():
    sc.check_identity_and_off("host")


@pytest.mark.parametrize("game,n,P", [("go", 5, 1), ("go", 5, 4), ("gomoku", 7, 1)])
def test_batch_search_with_a_host_eval_func(game, n, P):
    sc.check_batch_search("host", game, n, P)


def test_actor_with_random_symmetry_harvests_true_orientation_games():
    sc.check_actor_random("host")


def test_bad_modes_are_refused():
    sc.check_refusals("host")
