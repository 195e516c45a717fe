"""First-play urgency reduction on the host twin (CPU tier): the drivers of tests/fpu_checks.py, which tests/test_fpu_gpu.py runs on the
device."""
import pytest

import fpu_checks as fk


@pytest.mark.parametrize("r", [fk.KATAGO, fk.ZERO], ids=["katago", "zero"])
@pytest.mark.parametrize("root_noise", [True, False], ids=["noise", "plain"])
@pytest.mark.parametrize("shape,P", fk.CASES)
def test_engine_equals_the_restated_search(shape, P, root_noise, r):
    fk.check_restatement("host", shape, P, root_noise, r)


def test_reference_set_is_worth_comparing_with():
    fk.check_reference_set()


def test_off_is_the_parent():
    fk.check_off_is_the_parent("host")


def test_switch_in_the_middle_of_a_search():
    fk.check_switch_in_flight("host")


def test_case_that_needs_the_feature():
    fk.check_discriminating_case("host")


def test_with_forced_playouts():
    fk.check_with_forced_playouts("host")


def test_with_gumbel_root():
    fk.check_with_gumbel("host")


def test_leaf_symmetry():
    fk.check_leaf_symmetry("host")


def test_playout_cap_fast_moves_use_the_rule():
    fk.check_playout_cap("host")


@pytest.mark.parametrize("game,n,P", [("go", 5, 1), ("go", 5, 4), ("gomoku", 7, 1)])
def test_batch_search(game, n, P):
    fk.check_batch_search("host", game, n, P)


def test_resident_loop_equals_callback_loop():
    fk.check_resident_equals_callback("host")


def test_seeded_actor_is_reproducible():
    fk.check_seeded_actor("host")


def test_evaluation_games():
    fk.check_eval_games("host")


def test_refusals():
    fk.check_refusals("host")
