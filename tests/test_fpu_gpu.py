"""First-play urgency reduction on the device: the drivers of tests/fpu_checks.py against libazsp.so."""
import pytest

import fpu_checks as fk

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("r", [fk.KATAGO, fk.ZERO], ids=["katago", "zero"])
@pytest.mark.parametrize("root_noise", [True, False], ids=["noise", "plain"])
@pytest.mark.parametrize("shape,P", fk.CASES)
def test_engine_equals_the_restated_search(shape, P, root_noise, r):
    fk.check_restatement("gpu", shape, P, root_noise, r)


def test_off_is_the_parent():
    fk.check_off_is_the_parent("gpu")


def test_switch_in_the_middle_of_a_search():
    fk.check_switch_in_flight("gpu")


def test_case_that_needs_the_feature():
    fk.check_discriminating_case("gpu")


def test_with_forced_playouts():
    fk.check_with_forced_playouts("gpu")


def test_with_gumbel_root():
    fk.check_with_gumbel("gpu")


def test_leaf_symmetry():
    fk.check_leaf_symmetry("gpu")


def test_playout_cap_fast_moves_use_the_rule():
    fk.check_playout_cap("gpu")


@pytest.mark.parametrize("game,n,P", [("go", 5, 1), ("go", 5, 4), ("gomoku", 7, 1)])
def test_batch_search(game, n, P):
    fk.check_batch_search("gpu", game, n, P)


def test_resident_loop_equals_callback_loop():
    fk.check_resident_equals_callback("gpu")


def test_resident_loop_behind_a_device_evaluator():
    fk.check_resident_identity_gpu()


def test_seeded_actor_equals_the_host_twin():
    fk.check_seeded_actor("gpu")


def test_evaluation_games():
    fk.check_eval_games("gpu")


def test_refusals():
    fk.check_refusals("gpu")
