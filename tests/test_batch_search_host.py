"""CPU tier of the batched position search (host twin): azsp_set_states / azsp_begin_moves / azsp_read_searches, BatchSearch and
uct_search_many / parallel_uct_search_many.  The same drivers run on the device in test_batch_search_gpu.py."""
import pytest

import batch_search_checks as bc

GOLDENS = ["go5_p1_s40", "go5_p4_s48_resign", "go5_p8_s64", "gomoku7_p8_s64", "go9_p1_s50", "go5_p1_s40_det"]


@pytest.mark.parametrize("game,n,K,G", bc.SHAPES)
def test_set_states_equals_set_state_slot_by_slot(game, n, K, G):
    bc.check_set_states_equals_set_state("host", game, n, K, G)


def test_load_keep_and_idle_rows_in_the_middle_of_a_search():
    bc.check_actions_mixed_in_mid_search("host")


def test_refused_rows_report_their_code_and_leave_the_slot_idle():
    bc.check_refused_rows("host")


def test_begin_moves_per_slot_flags_noise_rows_and_skip():
    bc.check_begin_moves("host")
    bc.check_begin_moves("host", game="gomoku", n=7)


@pytest.mark.parametrize("device_route", [False, True], ids=["callback", "resident"])
@pytest.mark.parametrize("name", GOLDENS)
def test_all_games_of_a_golden_file_at_once_match_the_reference(name, device_route):
    bc.check_golden_games_at_once("host", name, device_route=device_route)


def test_batch_search_object():
    bc.check_batch_search_object("host")


def test_errors():
    bc.check_errors("host")
