"""CPU tier of the auxiliary training targets: the drivers of aux_checks.py on the host twin."""
import pytest

import aux_checks as ac


def test_the_flood_fill_restatement_on_known_boards():
    ac.check_restatement()


@pytest.mark.parametrize("n", [5, 9, 19])
def test_go_ownership_and_score_are_the_restatement(n):
    ac.check_go_ownership_and_score("host", n)


def test_a_resigned_game_carries_the_board_at_the_resignation():
    ac.check_resignation("host")


@pytest.mark.parametrize("reuse_tree", [0, 1])
def test_root_value_is_the_logged_root_q_as_float32(reuse_tree):
    ac.check_root_value("host", reuse_tree)


def test_both_staging_buffers_carry_their_own_ownership():
    ac.check_both_staging_buffers("host")


def test_nothing_else_moves_and_the_refusals():
    ac.check_nothing_else_moves("host")


def test_gomoku_ownership_is_the_final_board_and_score_is_z():
    ac.check_gomoku("host")


@pytest.mark.parametrize("n", [5, 9])
def test_replay_gathers_the_aux_rings_under_the_same_op(n):
    ac.check_replay("host", n)


def test_actor_leaves_the_aux_rows_in_last_harvest_aux():
    ac.check_actor("host")


def test_actor_reference_format_is_unchanged():
    ac.check_actor_reference_format("host")
