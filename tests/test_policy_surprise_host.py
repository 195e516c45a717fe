"""CPU tier of policy surprise weighting: the drivers of surprise_checks.py on the host twin."""
import pytest

import surprise_checks as sc


def test_the_restatements_on_known_values():
    sc.check_restatements()


@pytest.mark.parametrize("game,n", [("go", 5), ("go", 9), ("go", 19), ("gomoku", 7)])
def test_surprise_is_the_restated_kl(game, n):
    sc.check_surprise("host", game, n)


@pytest.mark.parametrize("variant", ["noise", "forced", "gumbel"])
def test_surprise_is_taken_on_the_recorded_target_against_the_raw_prior(variant):
    sc.check_surprise("host", "go", 5, variant)


@pytest.mark.parametrize("include_fast", [False, True])
@pytest.mark.parametrize("frac", [0.0, 0.5, 1.0])
def test_weights_are_the_restated_formula_bit_for_bit(frac, include_fast):
    sc.check_weights("host", frac, include_fast)


def test_a_game_without_surprise_is_weighted_uniformly():
    sc.check_zero_surprise_game("host")


def test_both_staging_buffers_are_weighted_by_their_own_sums():
    sc.check_both_staging_buffers("host")


def test_off_is_off_and_the_refusals():
    sc.check_off_is_off("host")


@pytest.mark.parametrize("aux", [False, True])
@pytest.mark.parametrize("n", [5, 9])
def test_weighted_add_is_the_repeated_rows_appended(n, aux):
    sc.check_weighted_add("host", n, aux)


def test_weighted_add_with_full_weights_is_keep_and_the_refusals():
    sc.check_weighted_add_rules("host")


def test_actor_leaves_surprise_and_weight_and_fills_a_replay():
    sc.check_actor("host")
