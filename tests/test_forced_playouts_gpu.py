"""Device tier of the forced playouts with policy-target pruning (azsp_set_forced_playouts): the drivers of forced_checks.py on libazsp.so."""
import pytest

import forced_checks as fc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("root_noise", [True, False])
@pytest.mark.parametrize("shape,P", fc.CASES)
def test_gpu_engine_equals_the_restated_search(shape, P, root_noise):
    fc.check_restatement("gpu", shape, P, root_noise)


@pytest.mark.parametrize("P,root_noise", [(1, False), (4, True)])
@pytest.mark.parametrize("k", fc.LARGE_FACTORS)
def test_gpu_search_with_a_very_large_factor_finishes_as_the_restated_search(k, P, root_noise):
    fc.check_large_factor("gpu", k, P, root_noise)


def test_gpu_off_is_the_parent_and_prune_target_0_records_the_logged_policy():
    fc.check_off_is_the_parent("gpu")


def test_gpu_forced_child_reaches_its_visits_where_the_plain_search_does_not():
    fc.check_discriminating_case("gpu")


@pytest.mark.parametrize("P", [1, 4])
def test_gpu_playout_cap_fast_moves_are_neither_forced_nor_pruned(P):
    fc.check_playout_cap("gpu", P)


def test_gpu_forced_search_under_a_leaf_symmetry():
    fc.check_leaf_symmetry("gpu")


@pytest.mark.parametrize("game,n,P", [("go", 5, 1), ("go", 5, 4), ("gomoku", 7, 1)])
def test_gpu_batch_search_target_pi_with_different_budgets(game, n, P):
    fc.check_batch_search("gpu", game, n, P)


def test_gpu_resident_loop_equals_the_callback_loop():
    fc.check_resident_equals_callback("gpu")


def test_gpu_resident_search_behind_a_device_evaluator_equals_the_callback_loop():
    fc.check_resident_identity_gpu()


def test_gpu_seeded_actor_without_injection_equals_the_host_twin():
    fc.check_seeded_actor("gpu")


def test_gpu_bad_factors_are_refused():
    fc.check_refusals("gpu")
