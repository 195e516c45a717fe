"""Device tier of the Gumbel root search (azsp_set_gumbel): the drivers of gumbel_checks.py on libazsp.so."""
import pytest

import gumbel_checks as gc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape,P,m,reuse", gc.CASES)
def test_gpu_engine_equals_the_restated_search(shape, P, m, reuse):
    gc.check_restatement("gpu", shape, P, m, reuse)


def test_gpu_sequential_halving_spends_the_budget_as_scheduled():
    gc.check_schedule("gpu")


def test_gpu_off_is_off():
    gc.check_off_is_off("gpu")


def test_gpu_bad_arguments_and_forced_playouts_next_to_it_are_refused():
    gc.check_refusals("gpu")


@pytest.mark.parametrize("game,n,P", gc.BATCH_CASES)
def test_gpu_batch_search_equals_the_restated_and_the_one_slot_searches(game, n, P):
    gc.check_batch_search("gpu", game, n, P)


@pytest.mark.parametrize("P", [1, 4])
def test_gpu_actor_samples_carry_the_target_and_fast_moves_the_plain_policy(P):
    gc.check_actor_samples("gpu", P)


def test_gpu_production_draws_follow_the_gumbel_law():
    gc.check_production_draws("gpu")


def test_gpu_searches_in_flight_end_under_their_rule_when_the_mode_is_switched_to_forced_playouts():
    gc.check_switch_in_flight("gpu")


def test_gpu_a_seeded_search_draws_the_rows_the_probe_hands_out():
    gc.check_search_draws_are_the_probed_rows("gpu")
