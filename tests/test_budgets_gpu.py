"""Device tier of the per-game simulation budgets and the playout-cap actor: the drivers of budget_checks.py on libazsp.so."""
import pytest

import budget_checks as bc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("game,n,P", [("go", 5, 1), ("go", 5, 4), ("gomoku", 7, 8)])
def test_gpu_mixed_budgets_equal_uniform_searches(game, n, P):
    bc.check_mixed_budgets_equal_uniform_searches("gpu", game, n, P)


def test_gpu_out_of_range_budgets_and_caps_are_refused():
    bc.check_refusals("gpu")


@pytest.mark.parametrize("P", [1, 4])
def test_gpu_uct_search_many_with_one_num_simulations_per_env(P):
    bc.check_uct_search_many_with_a_list("gpu", P)


@pytest.mark.parametrize("P", [1, 4])
def test_gpu_playout_cap_at_the_ends_equals_the_uncapped_actors(P):
    bc.check_cap_at_the_ends("gpu", P=P)


@pytest.mark.parametrize("P", [1, 4])
def test_gpu_playout_cap_classes_are_the_recomputed_draws(P):
    bc.check_cap_in_the_middle("gpu", P)


def test_gpu_replay_keeps_the_masked_rows_of_a_harvest():
    bc.check_replay_keeps_the_masked_rows("gpu")
