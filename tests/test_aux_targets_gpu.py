"""Device tier of the auxiliary training targets: the drivers of aux_checks.py on libazsp.so."""
import pytest

import aux_checks as ac

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", [5, 9, 19])
def test_gpu_go_ownership_and_score_are_the_restatement(n):
    ac.check_go_ownership_and_score("gpu", n)


def test_gpu_a_resigned_game_carries_the_board_at_the_resignation():
    ac.check_resignation("gpu")


@pytest.mark.parametrize("reuse_tree", [0, 1])
def test_gpu_root_value_is_the_logged_root_q_as_float32(reuse_tree):
    ac.check_root_value("gpu", reuse_tree)


def test_gpu_both_staging_buffers_carry_their_own_ownership():
    ac.check_both_staging_buffers("gpu")


def test_gpu_nothing_else_moves_and_the_refusals():
    ac.check_nothing_else_moves("gpu")


def test_gpu_gomoku_ownership_is_the_final_board_and_score_is_z():
    ac.check_gomoku("gpu")


@pytest.mark.parametrize("n", [5, 9])
def test_gpu_replay_gathers_the_aux_rings_under_the_same_op(n):
    ac.check_replay("gpu", n)


def test_gpu_actor_leaves_the_aux_rows_in_last_harvest_aux():
    ac.check_actor("gpu")


def test_gpu_actor_reference_format_is_unchanged():
    ac.check_actor_reference_format("gpu")
