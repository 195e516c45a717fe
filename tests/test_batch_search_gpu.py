"""Device tier of the batched position search: the drivers of test_batch_search_host.py on libazsp.so, the goldens limited to 12 moves
per game, and the batch against sequential uct_search calls with the product evaluator."""
import pytest

import batch_search_checks as bc

pytestmark = pytest.mark.gpu

GOLDENS = ["go5_p1_s40", "go5_p4_s48_resign", "go5_p8_s64", "gomoku7_p8_s64", "go9_p1_s50", "go5_p1_s40_det", "gomoku13_p1_s100", "go9_p8_s200"]


@pytest.mark.parametrize("game,n,K,G", bc.SHAPES)
def test_gpu_set_states_equals_set_state_slot_by_slot(game, n, K, G):
    bc.check_set_states_equals_set_state("gpu", game, n, K, G)


def test_gpu_load_keep_and_idle_rows_in_the_middle_of_a_search():
    bc.check_actions_mixed_in_mid_search("gpu")


def test_gpu_refused_rows_report_their_code_and_leave_the_slot_idle():
    bc.check_refused_rows("gpu")


def test_gpu_begin_moves_per_slot_flags_noise_rows_and_skip():
    bc.check_begin_moves("gpu")
    bc.check_begin_moves("gpu", game="gomoku", n=7)


@pytest.mark.parametrize("device_route", [False, True], ids=["callback", "resident"])
@pytest.mark.parametrize("name", GOLDENS)
def test_gpu_all_games_of_a_golden_file_at_once_match_the_reference(name, device_route):
    bc.check_golden_games_at_once("gpu", name, max_moves=12, device_route=device_route)


def test_gpu_batch_search_object():
    bc.check_batch_search_object("gpu")


def test_gpu_errors():
    bc.check_errors("gpu")


def test_gpu_batch_equals_sequential_uct_search_with_the_product_evaluator():
    bc.check_batch_equals_sequential_with_product_evaluator()
