"""Batched actor + sample gather, CPU tier (host twin engine, fp32 torch-CPU network, gloo)."""
import os
import subprocess
import sys

import pytest
import numpy as np
import torch

import engine_util as eu
from alpha_zero_amd import _abi
from alpha_zero_amd.core.network import AlphaZeroNet
from alpha_zero_amd.core.pipeline import SelfPlayActor


def _actor(game="go", n=5, G=8, sims=16, P=4, **kw):
    torch.manual_seed(1)
    A = n * n + (1 if game == "go" else 0)
    net = AlphaZeroNet((17, n, n), A, 1, 8, 8, gomoku=(game != "go"))
    return SelfPlayActor(net, game=game, board_size=n, num_games=G, num_simulations=sims, num_parallel=P, warm_up_steps=4,
                         device="cpu", net_dtype=torch.float32, use_graph=False, binding=eu.hosttwin_binding(), **kw)


def test_actor_emits_reference_shaped_games():
    a = _actor()
    got = []
    for _ in range(200):
        a.run_rounds(10)
        got += a.harvest()
        if len(got) >= 12:
            break
    assert len(got) >= 12
    for seq, stats in got:
        assert stats["game_length"] == len(seq) and 0 < len(seq) <= 50
        assert set(stats) == {"game_length", "game_result", "num_passes", "is_resign_disabled", "is_marked_for_resign", "is_could_won",
                              "marked_resign_player", "resign_threshold", "training_steps"}
        z = np.array([t.value for t in seq])
        black = np.array([t.state[16, 0, 0] for t in seq])
        assert seq[0].state.shape == (17, 5, 5) and seq[0].state.dtype == np.int8 and seq[0].pi_prob.shape == (26,)
        assert seq[0].pi_prob.dtype == np.float64 and abs(seq[0].pi_prob.sum() - 1) < 1e-5
        res = stats["game_result"]
        # z is +1 for the winner's samples, -1 for the loser's (pipeline.py:349-354)
        if res.startswith("B+"):
            assert np.all(z[black == 1] == 1) and np.all(z[black == 0] == -1)
        elif res.startswith("W+"):
            assert np.all(z[black == 1] == -1) and np.all(z[black == 0] == 1)
        # colours alternate and the first position is the empty board with black to move
        assert black[0] == 1 and not seq[0].state[:16].any()
    c = a.counters()
    assert c["games"] >= 12 and c["moves"] > 0 and c["stalls"] == 0


def test_actor_gomoku_and_weight_swap():
    a = _actor(game="gomoku", n=7, G=4, sims=12, P=2)
    a.run_rounds(30)
    net2 = AlphaZeroNet((17, 7, 7), 49, 1, 8, 8, gomoku=True)
    a.set_network(net2, training_steps=1000)
    got = []
    for _ in range(300):
        a.run_rounds(10)
        got += a.harvest()
        if len(got) >= 9:
            break
    assert len(got) >= 9
    tags = [stats["training_steps"] for _, stats in got]
    # games that were in progress at the swap keep the tag of the weights that STARTED them (pipeline.py:237 -> :271) and are
    # counted as straddling; every game started afterwards carries the new tag
    assert set(tags) <= {0, 1000} and 1000 in tags and tags.count(0) == a.straddled_games and a.straddled_games <= 4
    for seq, stats in got:
        assert set(stats) == {"game_length", "game_result", "training_steps"}
        assert seq[0].pi_prob.dtype == np.float32
        assert stats["game_result"] in ("B+1.0", "W+1.0", "DRAW")


def _assert_games_tile_the_samples(games):
    order = games[np.argsort(games[:, _abi.GR_START])]
    assert order[0, _abi.GR_START] == 0 and np.all(order[1:, _abi.GR_START] == np.cumsum(order[:-1, _abi.GR_LENGTH]))


def test_sample_gather_two_ranks_gloo(tmp_path):
    """N > 1 data path: finished-game tensors of every rank arrive on rank 0 in rank order (gloo, world_size 2)."""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gather_worker.py")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29533")
    procs = [subprocess.Popen([sys.executable, script, str(r), "2", str(tmp_path)], env=env) for r in range(2)]
    assert all(p.wait(timeout=300) == 0 for p in procs)
    out = np.load(os.path.join(str(tmp_path), "rank0.npz"))
    games = out["games"]
    assert len(games) >= 2 and out["states"].shape[0] == out["z"].shape[0] == out["pi"].shape[0] == games[:, _abi.GR_LENGTH].sum()
    # starts are rebased: games tile the sample range without overlap
    _assert_games_tile_the_samples(games)
    assert set(np.unique(games[:, _abi.GR_SLOT] >> _abi.GR_SLOT_RANK_SHIFT)) == {0, 1}
    # each rank's samples are byte-identical to what that rank harvested locally
    for r in range(2):
        eu.assert_rank_samples_gathered(out, r, np.load(os.path.join(str(tmp_path), f"local{r}.npz")))


def test_sample_gather_eight_ranks_gloo(tmp_path):
    """The 8-GPU data path on 8 gloo ranks (the only de-risking of the driver's 8-GPU run available without the node):
    uneven sample counts per rank, ranks that contribute zero samples to a gather (padded exchange), the `rank << GR_SLOT_RANK_SHIFT` slot tag for all
    eight ranks, rebased starts -- and every rank's samples byte-identical on rank 0 to what that rank harvested locally."""
    W = 8
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gather_worker.py")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29537", OMP_NUM_THREADS="1")
    procs = [subprocess.Popen([sys.executable, script, str(r), str(W), str(tmp_path)], env=env) for r in range(W)]
    assert all(p.wait(timeout=900) == 0 for p in procs)
    out = np.load(os.path.join(str(tmp_path), "rank0.npz"))
    games = out["games"]
    assert out["states"].shape[0] == out["z"].shape[0] == out["pi"].shape[0] == games[:, _abi.GR_LENGTH].sum()
    _assert_games_tile_the_samples(games)
    rank = games[:, _abi.GR_SLOT] >> _abi.GR_SLOT_RANK_SHIFT
    assert set(np.unique(rank)) == set(range(W)) and set(np.unique(games[:, _abi.GR_SLOT] & _abi.GR_SLOT_MASK)) <= set(range(4))
    counts = [int((rank == r).sum()) for r in range(W)]
    assert min(counts) >= 1 and len(set(counts)) > 1, counts  # uneven by construction (different budgets, sitting out)
    for r in range(W):
        eu.assert_rank_samples_gathered(out, r, np.load(os.path.join(str(tmp_path), f"local{r}.npz")))


def test_actor_loop_writes_reference_csv(tmp_path):
    """run_selfplay_actor_loop with logs_dir: actor{rank}.csv carries the reference's columns in its order
    (header of the reference's logs/go/9x9/actor0.csv), and the queue receives (game_seq, stats) with the same key order."""
    import csv
    import queue
    import threading

    from alpha_zero_amd.core.pipeline import run_selfplay_actor_loop
    from alpha_zero_amd.envs.go import GoEnv

    torch.manual_seed(1)
    net = AlphaZeroNet((17, 5, 5), 26, 1, 8, 8)
    env = GoEnv(board_size=5, _binding=eu.hosttwin_binding(), _device="cpu")
    q, stop = queue.Queue(), threading.Event()
    th = threading.Thread(target=run_selfplay_actor_loop, args=(
        3, 0, net, "cpu", q, env, 12, 4, 19652, 1.25, 4, 10, 0.1), kwargs=dict(
        logs_dir=str(tmp_path), save_sgf_dir=str(tmp_path), save_sgf_interval=1, stop_event=stop, num_games=8, net_dtype=torch.float32,
        harvest_every=20, binding=eu.hosttwin_binding()))
    th.start()
    first = q.get(timeout=120)
    stop.set()
    th.join(timeout=120)
    assert not th.is_alive()
    want = "datetime,game_length,game_result,num_passes,is_resign_disabled,is_marked_for_resign,is_could_won,marked_resign_player,resign_threshold,time_per_game,training_steps"
    rows = list(csv.reader(open(os.path.join(str(tmp_path), "actor0.csv"))))
    assert ",".join(rows[0]) == want and len(rows) >= 2 and len(rows[1]) == len(rows[0])
    assert list(first[1].keys()) == want.split(",")[1:]
    assert int(rows[1][1]) > 0 and rows[1][2][0] in "BWD"
    sgfs = sorted(f for f in os.listdir(str(tmp_path)) if f.endswith(".sgf"))  # pipeline.py:276-281: periodic SGF dumps
    assert sgfs and sgfs[0].startswith("actor0_")
    text = open(os.path.join(str(tmp_path), sgfs[0])).read()
    assert text.startswith("(;\nCA[UTF-8]\nAP[AlphaZeroMini_sgfgenerator]\nRU[Chinese]") and "SZ[5]" in text and text.endswith(")")


def check_per_game_actor_state(a, n_games=8):
    """pipeline.py:232-246: the resign threshold and the weights' training_steps are read when a game STARTS.  The actor begins
    with resignation off (-1, the learner's warm-up value pipeline.py:449-459), the threshold is raised while games are in
    progress, later lowered again: every game reports the threshold it started with, resigns only if that one allows it, and
    draws resign_disabled only while its threshold is > -1 (pipeline.py:244-246)."""
    G = a.cfg.num_games
    assert a.resign_threshold == -1.0
    a.run_rounds(6)                      # all first games are in progress with threshold -1
    a.set_resign_threshold(-0.3)
    a.set_network(a._net, training_steps=77) if hasattr(a, "_net") else None
    got = []
    for _ in range(400):
        a.run_rounds(10)
        got += a.harvest()
        if len(got) >= n_games + G:
            break
    assert len(got) >= n_games + G
    first, later = got[:G], got[G:]
    thr = [s["resign_threshold"] for _, s in got]
    assert set(thr) == {-1.0, -0.3}
    old = [s for _, s in got if s["resign_threshold"] == -1.0]
    new = [s for _, s in got if s["resign_threshold"] == -0.3]
    assert len(old) == G                                  # exactly the games that were running when the value changed
    assert all(s["is_resign_disabled"] and not s["is_marked_for_resign"] and not s["game_result"].endswith("+R") for s in old)
    assert any(not s["is_resign_disabled"] for s in new)   # the per-game draw happens once the threshold is > -1
    assert any(s["game_result"].endswith("+R") for s in new)  # and those games may resign
    assert all(s["is_resign_disabled"] for s in new if s["is_marked_for_resign"])
    return got


def test_per_game_resign_threshold_and_training_steps():
    a = _actor(G=6, sims=12, P=4, resign_threshold=-1.0, check_resign_after_steps=4, disable_resign_ratio=0.5)
    torch.manual_seed(2)
    a._net = AlphaZeroNet((17, 5, 5), 26, 1, 8, 8)
    got = check_per_game_actor_state(a, n_games=20)
    old = [s for _, s in got if s["resign_threshold"] == -1.0]
    new = [s for _, s in got if s["resign_threshold"] == -0.3]
    assert all(s["training_steps"] == 0 for s in old) and all(s["training_steps"] == 77 for s in new)
    assert a.straddled_games == 6
    # dropping instead of tagging
    b = _actor(G=4, sims=12, P=4)
    b.drop_straddling_games = True
    b.run_rounds(6)
    b.set_network(a._net, training_steps=5)
    out = []
    for _ in range(200):
        b.run_rounds(10)
        out += b.harvest()
        if len(out) >= 6:
            break
    assert b.straddled_games == 4 and all(s["training_steps"] == 5 for _, s in out)


def test_actor_loop_rereads_the_resign_threshold(tmp_path):
    """run_selfplay_actor_loop follows var_resign_threshold at run time (pipeline.py:241-242) and discards games while ckpt_event is
    set (pipeline.py:264-267)."""
    import multiprocessing as mp
    import queue
    import threading

    from alpha_zero_amd.core.pipeline import run_selfplay_actor_loop
    from alpha_zero_amd.envs.go import GoEnv

    torch.manual_seed(1)
    net = AlphaZeroNet((17, 5, 5), 26, 1, 8, 8)
    env = GoEnv(board_size=5, _binding=eu.hosttwin_binding(), _device="cpu")
    var_thr = mp.Value("d", -1.0)
    q, stop, ckpt = queue.Queue(), threading.Event(), threading.Event()
    th = threading.Thread(target=run_selfplay_actor_loop, args=(3, 0, net, "cpu", q, env, 12, 4, 19652, 1.25, 4, 4, 0.5), kwargs=dict(
        logs_dir=str(tmp_path), stop_event=stop, ckpt_event=ckpt, var_resign_threshold=var_thr, num_games=6, net_dtype=torch.float32,
        harvest_every=10, binding=eu.hosttwin_binding()))
    th.start()
    first = q.get(timeout=120)
    assert first[1]["resign_threshold"] == -1.0
    var_thr.value = -0.25
    seen = []
    for _ in range(400):
        seen.append(q.get(timeout=120)[1]["resign_threshold"])
        if seen[-1] == -0.25:
            break
    assert seen[-1] == -0.25
    ckpt.set()      # learner writes a checkpoint: nothing may reach the queue while the event is set
    import time
    time.sleep(1.0)
    while not q.empty():
        q.get()
    time.sleep(1.0)
    assert q.empty()
    ckpt.clear()
    q.get(timeout=120)
    stop.set()
    th.join(timeout=120)
    assert not th.is_alive()


def test_resign_controller_warm_up_and_finalizer_pool():
    from alpha_zero_amd.core import mcts_v2
    from alpha_zero_amd.core.evaluate import ResignController

    # pipeline.py:449-459, :533-536: -1 during the first no_resign_games games, reset to init when they are in
    rc = ResignController(-0.88, no_resign_games=3, reset_fp_interval=100, games_per_ckpt=100, disable_resign_ratio=0.1)
    assert rc.threshold == -1
    assert rc.on_game({}, 1) == -1 and rc.on_game({}, 2) == -1 and rc.on_game({}, 3) == -0.88
    assert ResignController(-1.0, 0, 100, 100, 0.1).threshold == -1
    assert ResignController(-0.9, 0, 100, 100, 0.1).threshold == -0.9

    # a consumed handle must not return its (still used) engine to the pool when it is garbage collected
    class Stub:
        key = ("stub",)

    mcts_v2._POOL.pop(("stub",), None)
    s = Stub()
    n1 = mcts_v2.Node(s, np.zeros((5, 5), np.int8), 1, 0)
    n1._alive = False
    n1._fin.detach()          # what _search does when the handle is handed back
    n2 = mcts_v2.Node(s, np.zeros((5, 5), np.int8), 2, 1)
    del n1
    import gc
    gc.collect()
    assert not mcts_v2._POOL.get(("stub",))           # the engine n2 uses is NOT in the pool
    del n2
    gc.collect()
    assert mcts_v2._POOL.get(("stub",)) == [s]         # dropping the live handle releases it, once
    mcts_v2._release(s)
    assert mcts_v2._POOL.get(("stub",)) == [s]
    mcts_v2._POOL.pop(("stub",), None)


def check_harvested_moves(a):
    """azsp_harvest_moves: the move list of every finished self-play game, replayed through the CPU oracle env, reproduces each
    recorded sample state, the game length, the pass count and the result string."""
    from oracle.envs import OracleGoEnv

    got = []
    for _ in range(300):
        a.run_rounds(10)
        got += a.harvest(with_moves=True)
        if len(got) >= 14:
            break
    assert len(got) >= 14
    resigned = 0
    for seq, stats, moves in got:
        env = OracleGoEnv(5)
        obs = env.reset()
        for i, t in enumerate(seq):
            assert np.array_equal(t.state, obs)  # the sample is the observation before move i
            if i < len(moves):
                obs, _, done, _ = env.step(moves[i])
        if len(moves) == len(seq) - 1:  # the last sample's mover resigned: not a history move (base.py:224-226)
            resigned += 1
            env.step(env.resign_move)
        else:
            assert len(moves) == len(seq)
        assert env.is_game_over() and env.get_result_string() == stats["game_result"] and env.steps == stats["game_length"]
        assert sum(1 for m in moves if m == 25) == stats["num_passes"]
        sgf = a.game_sgf(stats, moves, date="d")
        assert sgf.count(";B[") + sgf.count(";W[") == len(moves) and f"RE[{stats['game_result']}]" in sgf and "SZ[5]" in sgf
    assert resigned >= 1  # the resignation path was exercised


def test_harvested_moves_replay_to_the_samples_and_the_result():
    check_harvested_moves(_actor(G=6, sims=12, P=4, resign_threshold=-0.3, check_resign_after_steps=4, disable_resign_ratio=0.5))


def check_actor_loop(device, binding, tmp_path):
    """run_selfplay_actor_loop (pipeline.py:166-286): queue tuples (game_seq, stats) with the reference's key order,
    actor{rank}.csv with the reference's columns, checkpoint hot-swap through var_ckpt (file + training_steps tag), the
    threshold followed at run time, nothing queued while ckpt_event is set."""
    import csv
    import multiprocessing as mp
    import queue
    import threading
    import time

    import torch

    from alpha_zero_amd.core.network import AlphaZeroNet
    from alpha_zero_amd.core.pipeline import run_selfplay_actor_loop
    from alpha_zero_amd.core.replay import Transition
    from alpha_zero_amd.envs.go import GoEnv

    torch.manual_seed(1)
    net = AlphaZeroNet((17, 5, 5), 26, 1, 8, 8)
    torch.manual_seed(5)
    net2 = AlphaZeroNet((17, 5, 5), 26, 1, 8, 8)
    ck = os.path.join(str(tmp_path), "training_steps_500.ckpt")
    torch.save({"network": net2.state_dict(), "training_steps": 500}, ck)
    env = GoEnv(board_size=5, _binding=binding, _device=device)
    var_thr, var_ckpt = mp.Value("d", -1.0), mp.Array("c", 512)
    q, stop, ckpt_ev = queue.Queue(), threading.Event(), threading.Event()
    th = threading.Thread(target=run_selfplay_actor_loop, args=(3, 0, net, device, q, env, 12, 4, 19652, 1.25, 4, 4, 0.5), kwargs=dict(
        logs_dir=str(tmp_path), save_sgf_dir=str(tmp_path), save_sgf_interval=3, stop_event=stop, ckpt_event=ckpt_ev, var_ckpt=var_ckpt,
        var_resign_threshold=var_thr, num_games=8, net_dtype=torch.float32, harvest_every=10, binding=binding))
    th.start()
    try:
        seq, stats = q.get(timeout=300)
        want = "datetime,game_length,game_result,num_passes,is_resign_disabled,is_marked_for_resign,is_could_won,marked_resign_player,resign_threshold,time_per_game,training_steps"
        assert list(stats.keys()) == want.split(",")[1:]
        assert isinstance(seq[0], Transition) and seq[0].state.shape == (17, 5, 5) and seq[0].state.dtype == np.int8
        assert seq[0].pi_prob.dtype == np.float64 and seq[0].pi_prob.shape == (26,) and len(seq) == stats["game_length"]
        assert stats["training_steps"] == 0 and stats["resign_threshold"] == -1.0
        var_thr.value = -0.25
        var_ckpt.value = ck.encode("utf-8")
        tags = []
        for _ in range(2000):
            s = q.get(timeout=300)[1]
            tags.append((s["training_steps"], s["resign_threshold"]))
            if tags[-1] == (500, -0.25):
                break
        assert tags[-1] == (500, -0.25) and all(t in ((0, -1.0), (0, -0.25), (500, -0.25)) for t in tags)
        ckpt_ev.set()
        time.sleep(1.5)
        while not q.empty():
            q.get()
        time.sleep(1.5)
        assert q.empty()
        ckpt_ev.clear()
        q.get(timeout=300)
    finally:
        stop.set()
        th.join(timeout=300)
    assert not th.is_alive()
    rows = list(csv.reader(open(os.path.join(str(tmp_path), "actor0.csv"))))
    assert ",".join(rows[0]) == want and len(rows) >= 3 and all(len(r) == len(rows[0]) for r in rows[1:])
    assert {r[-1] for r in rows[1:]} <= {"0", "500"} and "500" in {r[-1] for r in rows[1:]}
    assert any(f.endswith(".sgf") for f in os.listdir(str(tmp_path)))


def test_actor_loop_hot_swap_threshold_and_ckpt_event(tmp_path):
    check_actor_loop("cpu", eu.hosttwin_binding(), tmp_path)


def test_game_range_rounds_equal_whole_batch_rounds():
    """azsp_select_range / azsp_expand_backup_range (host twin): rounds run as two disjoint game ranges, in either order, give exactly
    the games of whole-batch rounds -- the property SelfPlayActor's two half-batch streams rely on (mcts_v2.py:568-625 is per game).
    Ranges that do not start on a multiple of 32 games are refused."""
    def play(order):
        a = _actor(G=72, sims=12, P=4, seed=5)
        e = a.engine
        by_uid = {}
        for r in range(100):
            if order is None:
                a.run_round()
            else:
                for g0, g1 in order:
                    e.expand_backup(g0, g1)
                    e.select(g0, g1)
                a._forward()
            if (r + 1) % 20 == 0:
                st, pi, z, games = a.harvest_tensors()
                for row in games:
                    by_uid[int(row[_abi.GR_UID])] = tuple(t.clone() for t in eu.samples_of(row, st, pi, z)) + (np.delete(row, _abi.GR_START),)
        return by_uid, a.counters(), e

    whole, c0, _ = play(None)
    for order in ([(0, 32), (32, 72)], [(64, 72), (0, 64)]):
        part, c1, e = play(order)
        assert len(whole) >= 15 and whole.keys() == part.keys() and c0 == c1
        for uid, (s0, p0, z0, r0) in whole.items():
            s1, p1, z1, r1 = part[uid]
            assert torch.equal(s0, s1) and torch.equal(p0, p1) and torch.equal(z0, z1) and np.array_equal(r0, r1)
    for bad in ((8, 72), (0, 73), (32, 32), (-32, 32)):
        try:
            e.select(*bad)
        except Exception as ex:
            assert "azsp_select_range" in str(ex)
        else:
            raise AssertionError(f"range {bad} accepted")


def test_harvest_is_deterministic_and_capacity_keeps_a_prefix():
    """azsp_harvest hands out output rows by a scan in (rotating) slot order: two identical runs yield identical streams -- same games,
    same rows -- and a harvest without room for everything takes a prefix of that order and leaves the rest COMPLETE for the next call
    (nothing lost, nothing duplicated)."""
    def stream(cap_samples):
        a = _actor(G=40, sims=12, P=4, seed=9)
        out = []
        for r in range(9):
            a.run_rounds(20)
            st, pi, z, games = a.engine.harvest(sample_capacity=cap_samples, max_games=80)
            out.append((st.clone(), pi.clone(), z.clone(), games.copy()))
        return out

    big1, big2, small = stream(4000), stream(4000), stream(60)
    for (s1, p1, z1, g1), (s2, p2, z2, g2) in zip(big1, big2):
        assert torch.equal(s1, s2) and torch.equal(p1, p2) and torch.equal(z1, z2) and np.array_equal(g1, g2)
    assert sum(len(g) for *_, g in big1) > 20
    for st, pi, z, g in big1 + small:  # rows tile the output without gaps, in game-record order
        ln = g[:, _abi.GR_LENGTH]
        assert st.shape[0] == int(ln.sum()) and (len(g) == 0 or np.array_equal(g[:, _abi.GR_START], np.concatenate([[0], np.cumsum(ln)[:-1]])))
    # a capacity of 60 samples binds (several games of ~25 samples finish per harvest): never more than 60 rows, games only delayed
    assert all(st.shape[0] <= 60 for st, *_ in small) and any(len(g) >= 2 for *_, g in small)
    uid_big = [int(u) for *_, g in big1 for u in g[:, _abi.GR_UID]]
    uid_small = [int(u) for *_, g in small for u in g[:, _abi.GR_UID]]
    assert len(set(uid_small)) == len(uid_small) and len(uid_small) >= 8  # every game at most once
    first = {int(row[_abi.GR_UID]): eu.samples_of(row, st) for st, _, _, g in big1 for row in g}
    for st, _, _, g in small:  # a game harvested late is the same game (content depends on seed, slot, uid only)
        for row in g:
            u = int(row[_abi.GR_UID])
            if u in first and u < 40:  # first game of a slot: not yet affected by the slots that stalled on a full harvest
                assert torch.equal(eu.samples_of(row, st), first[u])
    assert set(uid_small[:8]) <= set(uid_big)


@pytest.mark.parametrize("n_samples", [1, 2, 7])
@pytest.mark.parametrize("shape,A", [((17, 9, 9), 82), ((17, 13, 13), 169), ((17, 19, 19), 362), ((17, 5, 5), 26)])
def test_pack_unpack_round_trip_every_row_count(n_samples, shape, A):
    """The wire format of the sample gather (core/gather.py) round-trips bit for bit for ANY sample count -- a single sample included:
    at 9x9 Go a row is 173 + 328 + 4 = 505 bytes (not a multiple of 4), and a [1, k] slice of such a row must still become a dense,
    4-byte aligned buffer before it is viewed as float32 (one-sample harvests crashed the replay rank)."""
    from alpha_zero_amd.core.gather import pack_samples, unpack_samples

    g = torch.Generator().manual_seed(n_samples * 1000 + A)
    st = (torch.rand((n_samples,) + shape, generator=g) < 0.3).to(torch.int8)
    pi = torch.rand((n_samples, A), generator=g)
    z = torch.rand((n_samples,), generator=g) * 2 - 1
    rows = pack_samples(st, pi, z)
    assert rows.shape == (n_samples, (int(np.prod(shape)) + 7) // 8 + 4 * A + 4)
    # the receiving side sees the rows as a slice of one flat byte buffer (gather_samples: out[r][: n * rb].reshape(n, rb))
    flat = torch.cat([rows.reshape(-1), torch.zeros(13, dtype=torch.uint8)])
    s2, p2, z2 = unpack_samples(flat[: rows.numel()].reshape(n_samples, rows.shape[1]), shape, A)
    assert torch.equal(s2, st) and torch.equal(p2, pi) and torch.equal(z2, z)


def test_clamp_window_bookkeeping():
    """ClampWindow (VERDICT r5 Weak #1): after a range event at a poll, the games in progress and the finished games not handed out yet
    are suspect; games that finished before an earlier harvest, and games that start after the poll, are not."""
    from alpha_zero_amd.core.pipeline import ClampWindow

    G = 4
    cw = ClampWindow(G)
    uid = lambda slot, idx: idx * G + slot  # noqa: E731  (az_engine.h: uid = games_done * G + slot)
    assert not cw.mask([uid(0, 0), uid(1, 0), uid(0, 1)]).any()          # clean harvest: slot 0 handed out games 0-1, slot 1 game 0
    assert list(cw.next_unharvested) == [2, 1, 0, 0]
    cw.on_event([3, 1, 0, 2])                                               # slot 0 plays its game 3 (game 2 finished, not harvested), ...
    m = cw.mask([uid(0, 2), uid(0, 3), uid(1, 1), uid(3, 0), uid(3, 1), uid(3, 2), uid(2, 0)])
    assert list(m) == [True, True, True, True, True, True, True]
    m = cw.mask([uid(0, 4), uid(1, 2), uid(3, 3), uid(2, 1)])               # games that started after the repair
    assert not m.any() and cw.events == 1
    assert (cw.hi == -1).all()                                              # all intervals used up
    cw.on_event([5, 3, 2, 4])                                               # a second event later: only what is in flight / unharvested now
    assert list(cw.mask([uid(0, 5), uid(1, 3)])) == [True, True] and not cw.mask([uid(0, 6)]).any()


def test_actor_marks_or_drops_the_games_of_a_clamp_window():
    """SelfPlayActor.harvest() on the host twin with a clamp event injected between two harvests (the device poll itself is GPU-only):
    every game of the window carries stats['evaluator_clamped'] (or is dropped with drop_clamped_games), no other game does, and the
    reference's stats keys are untouched on clean games."""
    for drop in (False, True):
        a = _actor(G=8)
        a.drop_clamped_games = drop
        take = a.harvest
        clean = []
        for _ in range(12):
            a.run_rounds(10)
            clean += take()
        assert clean and not any("evaluator_clamped" in st for _, st in clean) and a.clamped_games == 0
        front = a.clamp_window.next_unharvested.copy()
        a.run_rounds(7)
        done = a.engine.status()[0][:, _abi.STC_GAMES_DONE].copy()
        a.clamp_window.on_event(done)  # what _check_evaluator_range does when the device record shows an event
        expect = int(sum(max(0, int(done[s]) - int(front[s]) + 1) for s in range(8)))  # per slot: unharvested finished games + the one in progress
        after = []
        for _ in range(400):
            a.run_rounds(10)
            after += take()
            if (a.clamp_window.hi == -1).all() and len(after) > expect + 8:
                break
        assert (a.clamp_window.hi == -1).all()
        marked = [st for _, st in after if st.get("evaluator_clamped")]
        assert a.clamped_games == expect, (a.clamped_games, expect)
        if drop:
            assert not marked and len(after) > 8  # dropped, the rest flows on
        else:
            assert len(marked) == expect and len(after) > expect
            keys = {"game_length", "game_result", "num_passes", "is_resign_disabled", "is_marked_for_resign", "is_could_won", "marked_resign_player",
                    "resign_threshold", "training_steps"}
            assert all(set(st) == keys | {"evaluator_clamped"} for st in marked) and all(set(st) == keys for _, st in after if not st.get("evaluator_clamped"))
