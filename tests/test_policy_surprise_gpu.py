"""Device tier of policy surprise weighting: the drivers of surprise_checks.py on libazsp.so."""
import pytest

import surprise_checks as sc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("game,n", [("go", 5), ("go", 9), ("go", 19), ("gomoku", 7)])
def test_gpu_surprise_is_the_restated_kl(game, n):
    sc.check_surprise("gpu", game, n)


@pytest.mark.parametrize("variant", ["noise", "forced", "gumbel"])
def test_gpu_surprise_is_taken_on_the_recorded_target_against_the_raw_prior(variant):
    sc.check_surprise("gpu", "go", 5, variant)


@pytest.mark.parametrize("include_fast", [False, True])
@pytest.mark.parametrize("frac", [0.0, 0.5, 1.0])
def test_gpu_weights_are_the_restated_formula_bit_for_bit(frac, include_fast):
    sc.check_weights("gpu", frac, include_fast)


def test_gpu_a_game_without_surprise_is_weighted_uniformly():
    sc.check_zero_surprise_game("gpu")


def test_gpu_both_staging_buffers_are_weighted_by_their_own_sums():
    sc.check_both_staging_buffers("gpu")


def test_gpu_off_is_off_and_the_refusals():
    sc.check_off_is_off("gpu")


@pytest.mark.parametrize("aux", [False, True])
@pytest.mark.parametrize("n", [5, 9])
def test_gpu_weighted_add_is_the_repeated_rows_appended(n, aux):
    sc.check_weighted_add("gpu", n, aux)


def test_gpu_weighted_add_with_full_weights_is_keep_and_the_refusals():
    sc.check_weighted_add_rules("gpu")


def test_gpu_actor_leaves_surprise_and_weight_and_fills_a_replay():
    sc.check_actor("gpu")
