"""Device tier of the decided-game visit reduction: the drivers of reduce_checks.py on libazsp.so."""
import pytest

import reduce_checks as rc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape,P", rc.CASES)
def test_gpu_the_search_is_the_restated_search(shape, P):
    rc.check_restatement("gpu", shape, P)


@pytest.mark.parametrize("shape,P,rule", rc.EXTRA_CASES)
def test_gpu_moves_that_owe_no_simulation_are_the_restated_moves(shape, P, rule):
    rc.check_restatement("gpu", shape, P, rule)


@pytest.mark.parametrize("game,n,P,cap", [("go", 5, 1, None), ("go", 5, 2, (2, 0.5)), ("go", 9, 4, None), ("gomoku", 7, 1, None)])
def test_gpu_budgets_bases_and_the_counter_follow_from_the_move_log(game, n, P, cap):
    rc.check_log("gpu", game, n, P, cap)


@pytest.mark.parametrize("include_fast", [False, True])
@pytest.mark.parametrize("frac", [0.0, 0.5])
def test_gpu_weights_are_the_restated_formula_bit_for_bit(frac, include_fast):
    rc.check_weights("gpu", frac, include_fast)


def test_gpu_the_rule_alone_weights_base_times_class():
    rc.check_weights_alone("gpu")


def test_gpu_a_rule_that_never_fires_leaves_the_surprise_weights():
    rc.check_never_firing_weights("gpu")


def test_gpu_off_is_off():
    rc.check_off_is_off("gpu")


def test_gpu_the_refusals():
    rc.check_refusals("gpu")


def test_gpu_with_forced_playouts():
    rc.check_with_forced_playouts("gpu")


def test_gpu_with_a_gumbel_root_the_schedule_is_built_from_the_reduced_budget():
    rc.check_with_gumbel("gpu")


def test_gpu_with_fpu_reduction():
    rc.check_with_fpu("gpu")


def test_gpu_full_is_the_slots_own_budget():
    rc.check_slot_budgets("gpu")


def test_gpu_turned_on_between_two_moves_of_running_games():
    rc.check_switch_in_flight("gpu", None, rc.RULE)


def test_gpu_lookback_changed_between_two_moves_of_running_games():
    rc.check_switch_in_flight("gpu", (0.5, 3, 4, 0.25), (0.5, 1, 4, 0.25))


def test_gpu_both_staging_buffers_carry_their_own_bases():
    rc.check_both_staging_buffers("gpu")


def test_gpu_actor_leaves_base_and_weight_and_fills_a_replay():
    rc.check_actor("gpu")


def test_gpu_actor_with_the_rule_alone():
    rc.check_actor_alone("gpu")


def test_gpu_a_seeded_actor_is_reproducible_and_equals_the_host_twin():
    dev, host = rc.check_seeded_actor("gpu"), rc.check_seeded_actor("host")
    for k in dev:
        assert dev[k].tobytes() == host[k].tobytes(), k
