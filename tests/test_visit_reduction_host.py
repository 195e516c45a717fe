"""CPU tier of the decided-game visit reduction: the drivers of reduce_checks.py on the host twin."""
import pytest

import reduce_checks as rc


def test_the_restatements_on_known_values():
    rc.check_restatements()


def test_the_reference_set_is_worth_comparing_with():
    rc.check_reference_set()


@pytest.mark.parametrize("shape,P", rc.CASES)
def test_the_search_is_the_restated_search(shape, P):
    rc.check_restatement("host", shape, P)


@pytest.mark.parametrize("shape,P,rule", rc.EXTRA_CASES)
def test_moves_that_owe_no_simulation_are_the_restated_moves(shape, P, rule):
    rc.check_restatement("host", shape, P, rule)


@pytest.mark.parametrize("game,n,P,cap", [("go", 5, 1, None), ("go", 5, 2, (2, 0.5)), ("go", 9, 4, None), ("gomoku", 7, 1, None)])
def test_budgets_bases_and_the_counter_follow_from_the_move_log(game, n, P, cap):
    rc.check_log("host", game, n, P, cap)


@pytest.mark.parametrize("include_fast", [False, True])
@pytest.mark.parametrize("frac", [0.0, 0.5])
def test_weights_are_the_restated_formula_bit_for_bit(frac, include_fast):
    rc.check_weights("host", frac, include_fast)


def test_the_rule_alone_weights_base_times_class():
    rc.check_weights_alone("host")


def test_a_rule_that_never_fires_leaves_the_surprise_weights():
    rc.check_never_firing_weights("host")


def test_off_is_off():
    rc.check_off_is_off("host")


def test_the_refusals():
    rc.check_refusals("host")


def test_with_forced_playouts():
    rc.check_with_forced_playouts("host")


def test_with_a_gumbel_root_the_schedule_is_built_from_the_reduced_budget():
    rc.check_with_gumbel("host")


def test_with_fpu_reduction():
    rc.check_with_fpu("host")


def test_full_is_the_slots_own_budget():
    rc.check_slot_budgets("host")


def test_turned_on_between_two_moves_of_running_games():
    rc.check_switch_in_flight("host", None, rc.RULE)


def test_lookback_changed_between_two_moves_of_running_games():
    rc.check_switch_in_flight("host", (0.5, 3, 4, 0.25), (0.5, 1, 4, 0.25))


def test_both_staging_buffers_carry_their_own_bases():
    rc.check_both_staging_buffers("host")


def test_actor_leaves_base_and_weight_and_fills_a_replay():
    rc.check_actor("host")


def test_actor_with_the_rule_alone():
    rc.check_actor_alone("host")


def test_a_seeded_actor_is_reproducible():
    rc.check_seeded_actor("host")
