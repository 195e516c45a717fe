"""CPU tier of the forced playouts with policy-target pruning (azsp_set_forced_playouts): the drivers of forced_checks.py on the host twin."""
import pytest

import forced_checks as fc


@pytest.mark.parametrize("root_noise", [True, False])
@pytest.mark.parametrize("shape,P", fc.CASES)
def test_engine_equals_the_restated_search(shape, P, root_noise):
    fc.check_restatement("host", shape, P, root_noise)


def test_reference_set_has_pruned_targets_and_children_pruned_to_zero():
    """Of the restated searches alone, without the engine: the set the engine is compared with is not vacuous."""
    fc.check_pruning_is_not_vacuous()


@pytest.mark.parametrize("root_noise", [True, False])
@pytest.mark.parametrize("P", [1, 4])
@pytest.mark.parametrize("k", fc.LARGE_FACTORS)
def test_search_with_a_very_large_factor_finishes_as_the_restated_search(k, P, root_noise):
    fc.check_large_factor("host", k, P, root_noise)


def test_off_is_the_parent_and_prune_target_0_records_the_logged_policy():
    fc.check_off_is_the_parent("host")


def test_forced_child_reaches_its_visits_where_the_plain_search_does_not():
    fc.check_discriminating_case("host")


@pytest.mark.parametrize("P", [1, 4])
def test_playout_cap_fast_moves_are_neither_forced_nor_pruned(P):
    fc.check_playout_cap("host", P)


def test_forced_search_under_a_leaf_symmetry():
    fc.check_leaf_symmetry("host")


@pytest.mark.parametrize("game,n,P", [("go", 5, 1), ("go", 5, 4), ("gomoku", 7, 1)])
def test_batch_search_target_pi_with_different_budgets(game, n, P):
    fc.check_batch_search("host", game, n, P)


def test_resident_loop_equals_the_callback_loop():
    fc.check_resident_equals_callback("host")


def test_seeded_actor_without_injection_is_reproducible():
    fc.check_seeded_actor("host")


def test_bad_factors_are_refused():
    fc.check_refusals("host")
