"""CPU tier of the Gumbel root search (azsp_set_gumbel): the drivers of gumbel_checks.py on the host twin."""
import pytest

import gumbel_checks as gc


def test_considered_visit_sequence_equals_the_list_built_phase_by_phase():
    gc.check_considered_visits()


def test_every_root_decision_of_the_restated_cases_is_clear_by_the_margin():
    """Of the restated searches alone, without the engine."""
    gc.check_margins()


@pytest.mark.parametrize("shape,P,m,reuse", gc.CASES)
def test_engine_equals_the_restated_search(shape, P, m, reuse):
    gc.check_restatement("host", shape, P, m, reuse)


def test_sequential_halving_spends_the_budget_as_scheduled():
    gc.check_schedule("host")


def test_off_is_off():
    gc.check_off_is_off("host")


def test_bad_arguments_and_forced_playouts_next_to_it_are_refused():
    gc.check_refusals("host")


@pytest.mark.parametrize("game,n,P", gc.BATCH_CASES)
def test_batch_search_equals_the_restated_and_the_one_slot_searches(game, n, P):
    gc.check_batch_search("host", game, n, P)


@pytest.mark.parametrize("P", [1, 4])
def test_actor_samples_carry_the_target_and_fast_moves_the_plain_policy(P):
    gc.check_actor_samples("host", P)


def test_production_draws_follow_the_gumbel_law():
    gc.check_production_draws("host")


def test_searches_in_flight_end_under_their_rule_when_the_mode_is_switched_to_forced_playouts():
    gc.check_switch_in_flight("host")


def test_a_seeded_search_draws_the_rows_the_probe_hands_out():
    gc.check_search_draws_are_the_probed_rows("host")


def test_root_decisions_of_the_restated_schedule_and_batch_searches_are_clear_by_the_margin():
    """Of the restated searches alone, without the engine."""
    gc.check_schedule_margins()
    gc.check_batch_margins()
