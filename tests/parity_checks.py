"""Assertions shared by the host-twin (CPU) and GPU parity tests."""
import json

import numpy as np

import engine_util as eu
from alpha_zero_amd import _abi
import golden_mcts
from alpha_zero_amd.core.pipeline import game_stats_from_row
from synth_eval import eval_batch


def check_go_file(kind, path, n, chunk=2048):
    g = np.load(path)
    off, mv = g["offsets"], g["moves"]
    lists = [mv[off[i]:off[i + 1]].astype(np.int32) for i in range(len(off) - 1)]
    bad = []
    for c0 in range(0, len(lists), chunk):
        for j, (k, ds, do, fin) in enumerate(zip(*eu.replay_env_batch(kind, "go", n, lists[c0:c0 + chunk]))):
            i = c0 + j
            ok = (k == len(lists[i]) and ds == g["state_digest"][i].tobytes() and do == g["obs_digest"][i].tobytes()
                  and (fin[_abi.ENV_AREA_BLACK], fin[_abi.ENV_AREA_WHITE]) == tuple(g["areas"][i]))
            if not ok:
                bad.append(i)
    return bad, len(lists)


def check_gomoku_file(kind, path):
    g = np.load(path)
    off, mv = g["offsets"], g["moves"]
    groups = {}
    for i in range(len(off) - 1):
        groups.setdefault(tuple(int(x) for x in g["meta"][i][:2]), []).append(i)
    bad = []
    for (size, ntw), ids in groups.items():
        lists = [mv[off[i]:off[i + 1]].astype(np.int32) for i in ids]
        for i, k, ds, do, fin in zip(ids, *eu.replay_env_batch(kind, "gomoku", size, lists, num_to_win=ntw)):
            ok = (k == off[i + 1] - off[i] and ds == g["state_digest"][i].tobytes() and do == g["obs_digest"][i].tobytes()
                  and fin[_abi.ENV_WINNER] == g["meta"][i][2] and fin[_abi.ENV_REWARD] == g["meta"][i][3])
            if not ok:
                bad.append(i)
    return bad, len(off) - 1


def check_mcts_golden(kind, name, feature_dtype=_abi.FEAT_I8, prefix="mcts_"):
    """Batched actor with the recorded randomness injected vs the reference's outputs (prefix="stack_mcts_": the goldens at num_stack
    K < 8).  Bit-exact: visit counts, chosen moves, root_Q, best_child_Q, evaluation counts, (Go) pi as float64, the (state, pi, z)
    samples of finished games with 2K+1 planes and their stats.  Gomoku pi (float32 in the reference, platform-dependent np.power)
    <= 1e-6.  Returns (engine counters, number of finished games)."""
    G = golden_mcts.MctsGolden(name, prefix)
    g, cfg = G.g, G.cfg
    logs, (states, pis, zs, games), n_evals, counters, _ = eu.run_golden_selfplay(kind, G, eval_batch, feature_dtype)
    for gi in range(cfg["games"]):
        ix = G.moves_of_game(gi)
        for k, i in enumerate(ix):
            L = logs[gi][k]
            where = (name, gi, k)
            assert np.array_equal(L["child_N"], g["child_N"][i]), where
            assert L["move"] == g["move"][i], where
            assert L["root_q"] == g["root_q"][i] and L["child_q"] == g["child_q"][i], where
            if cfg["game"] == "go":
                assert np.array_equal(L["pi"], g["pi"][i]), where
            else:
                assert np.abs(L["pi"] - g["pi"][i]).max() <= 1e-6, where
            assert n_evals[gi, k] == g["n_evals"][i], where
    assert states.shape[1] == 2 * G.K + 1
    by_slot = {int(row[_abi.GR_SLOT]): row for row in games}
    finished = 0
    for gi in range(cfg["games"]):
        if not G.finished(gi):
            assert gi not in by_slot
            continue
        finished += 1
        st, gp, gz, gstats = G.samples(gi)
        row = by_slot[gi]
        est, epi, ez = eu.samples_of(row, states, pis, zs)
        assert len(est) == len(st)
        assert np.array_equal(est, st)
        assert np.array_equal(ez, gz.astype(np.float32))
        if cfg["game"] == "go":
            assert np.array_equal(epi, gp.astype(np.float32))
        else:
            assert np.abs(epi - gp).max() <= 1e-6
        stats = game_stats_from_row(row, game=cfg["game"], komi=7.5, resign_threshold=cfg.get("resign_threshold", -1.0))
        assert json.loads(json.dumps(stats)) == gstats, (stats, gstats)
    return counters, finished
