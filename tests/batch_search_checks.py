"""Shared drivers of the batched position search (azsp_set_states / azsp_begin_moves / azsp_read_searches, core/batch_search.py,
uct_search_many): the same functions run on the host twin (CPU tier) and on the device (`-m gpu`)."""
import functools

import numpy as np
import pytest
import torch

import dropin_checks as dc
import engine_util as eu
import golden_mcts
from alpha_zero_amd import _abi
from alpha_zero_amd.core.batch_search import BatchSearch, env_position
from alpha_zero_amd.core.engine import Engine, EngineConfig
from synth_eval import eval_batch, make_eval_func

# (game, board size, num_stack, G): every ballot / padding shape (Go 5x5: 25 of 64 lanes, 9x9: a partial second word, 19x19: 361 = 5 * 64
# + 41; Gomoku 7 / 13 / 15), history depths 1 / 4 / 8 with hist_boards = num_stack, and G = 1, 3, 5, 6 (a workgroup is four games)
SHAPES = [("go", 5, 8, 6), ("go", 9, 4, 5), ("go", 19, 1, 3), ("go", 9, 8, 1), ("gomoku", 7, 8, 1), ("gomoku", 13, 4, 6), ("gomoku", 15, 1, 3)]
# seeds of the random games the positions come from, chosen on the CPU so that each Go game has a ko, a pass and a capture
SEEDS = {("go", 5): (6, 48), ("go", 9): (3, 150), ("go", 19): (4, 700), ("gomoku", 7): (1, 40), ("gomoku", 13): (1, 120), ("gomoku", 15): (1, 160)}


@functools.lru_cache(maxsize=None)
def position_pool(game, n, K):
    """Six positions (board, hist[K], pos row) out of ONE seeded random game played through the env classes (host twin: the rules are
    the engine's, the same on both tiers).  Go: [a ko position, one right after a pass, one with captures and no ko, one with white to
    move, mid-game, the last]; Gomoku: plies spread over the game, white to move among them."""
    seed, plies = SEEDS[(game, n)]
    env = dc.make_env("host", game, n, num_stack=K)
    rng = np.random.Generator(np.random.PCG64(seed))
    snaps = []
    for _ in range(plies):
        legal = np.flatnonzero(env.legal_actions[: n * n])
        last_pass = game == "go" and len(env.history) > 0 and env.history[-1].move == env.pass_move
        if game == "go" and (len(legal) == 0 or (rng.random() < 0.03 and not last_pass)):
            a = n * n
        elif len(legal) == 0:
            break
        else:
            a = int(legal[rng.integers(len(legal))])
        env.step(a)
        if env.is_game_over():
            break
        snaps.append(env_position(env))
    col = lambda c: np.array([s[2][c] for s in snaps])  # noqa: E731
    white = col(_abi.PS_TO_PLAY) != 1
    if game == "go":
        ko, caps = col(_abi.PS_KO) >= 0, (col(_abi.PS_CAPS_BLACK) + col(_abi.PS_CAPS_WHITE)) > 0
        first = lambda m: int(np.flatnonzero(m)[0])  # noqa: E731
        pick = [first(ko), first(col(_abi.PS_LAST_PASS) == 1), first(caps & ~ko), first(white & caps), len(snaps) // 2, len(snaps) - 1]
    else:
        pick = [len(snaps) * k // 6 + (k % 2) for k in range(6)]
    return [snaps[i] for i in pick]


def positions(game, n, K, G):
    pool = position_pool(game, n, K)
    pos = [pool[i % len(pool)] for i in range(G)]
    return np.stack([p[0] for p in pos]), np.stack([p[1] for p in pos]), np.stack([p[2] for p in pos])


def assert_covers_the_rules_cases(pos):
    """The position set holds a ko position, one right after a pass, one with captures and one with white to move."""
    assert (pos[:, _abi.PS_KO] >= 0).any() and (pos[:, _abi.PS_LAST_PASS] == 1).any()
    assert ((pos[:, _abi.PS_CAPS_BLACK] + pos[:, _abi.PS_CAPS_WHITE]) > 0).any() and (pos[:, _abi.PS_TO_PLAY] != 1).any()


def make_engine(kind, game, n, K, G, P=2, sims=40, root_noise=False, **kw):
    b, dev = eu.backend(kind)
    return Engine(b, EngineConfig(game=game, board_size=n, num_games=G, num_parallel=P, num_simulations=sims, num_stack=K, stop_after_move=True,
                                  feature_dtype=_abi.FEAT_I8, root_noise=root_noise, seed=7, **kw), device=dev)


def load_one_by_one(eng, boards, hist, pos, slots=None):
    for i, g in enumerate(range(len(boards)) if slots is None else slots):
        r = pos[i]
        eng.set_state(g, boards[i], hist[i], int(r[_abi.PS_TO_PLAY]), int(r[_abi.PS_STEPS]), int(r[_abi.PS_KO]), bool(r[_abi.PS_LAST_PASS]),
                      (int(r[_abi.PS_CAPS_BLACK]), int(r[_abi.PS_CAPS_WHITE])))


def snapshot(eng):
    """(status, q, valid, decoded feature rows of the valid rows) of an engine between two rounds."""
    st, q = eng.status()
    valid = eng.valid.cpu().numpy().astype(bool)
    return st, q, valid, eu.decode_features(eng)


def play_round(eng, snap):
    """Evaluate the valid rows of `snap` with the synthetic evaluator and run one round (expand / backup, select)."""
    _, _, valid, feats = snap
    pri = np.zeros((eng.rows, eng.A), dtype=np.float32)
    val = np.zeros(eng.rows, dtype=np.float32)
    rows = np.flatnonzero(valid)
    if len(rows):
        pri[rows], val[rows] = eval_batch(feats[rows], eng.A)
    eng.priors.copy_(torch.from_numpy(pri))
    eng.values.copy_(torch.from_numpy(val))
    eng.round()


def assert_same_snapshot(a, b, games=None, P=1, where=None):
    """Two snapshots agree (on the given games): status, Q, valid flags and the feature rows the engine asked to be evaluated."""
    games = np.arange(a[0].shape[0]) if games is None else np.asarray(games)
    rows = (games[:, None] * P + np.arange(P)[None, :]).reshape(-1)
    assert np.array_equal(a[0][games], b[0][games]), (where, a[0][games], b[0][games])
    assert np.array_equal(a[1][games].view(np.int64), b[1][games].view(np.int64)), where
    assert np.array_equal(a[2][rows], b[2][rows]), where
    rows = rows[a[2][rows]]
    assert np.array_equal(a[3][rows], b[3][rows]), where


def assert_same_searches(ea, eb, slots_a=None, slots_b=None):
    """get_search / status of the slots agree bit for bit between two engines."""
    slots_a = range(ea.G) if slots_a is None else slots_a
    slots_b = slots_a if slots_b is None else slots_b
    sa, qa = ea.status()
    sb, qb = eb.status()
    for ga, gb in zip(slots_a, slots_b):
        pa, pb = ea.get_search(ga, 0), eb.get_search(gb, 0)
        assert pa[0].tobytes() == pb[0].tobytes() and pa[1].tobytes() == pb[1].tobytes(), (ga, gb)
        assert np.array_equal(sa[ga], sb[gb]) and qa[ga].tobytes() == qb[gb].tobytes(), (ga, gb, sa[ga], sb[gb])


def run_until_done(engines, slots=None, min_rounds=0, max_rounds=400, compare=None):
    """Rounds on all `engines` in step until the given slots of the first one are MOVE_DONE (and at least min_rounds were played);
    compare(round, snapshots) sees the engines' snapshots before every round."""
    for it in range(max_rounds):
        snaps = [snapshot(e) for e in engines]
        if compare is not None:
            compare(it, snaps)
        st = snaps[0][0][:, _abi.STC_STATUS] if slots is None else snaps[0][0][list(slots), _abi.STC_STATUS]
        if it >= min_rounds and np.all(st == _abi.ST_MOVE_DONE):
            return it
        for e, s in zip(engines, snaps):
            play_round(e, s)
    raise AssertionError("the searches did not finish")


# ---------------------------------------------------------------------------------------------------
# 1. set_states == G x set_state
# ---------------------------------------------------------------------------------------------------
def check_set_states_equals_set_state(kind, game, n, K, G):
    boards, hist, pos = positions(game, n, K, G)
    assert hist.shape[1] == K
    if game == "go" and G >= 3:
        assert_covers_the_rules_cases(np.stack([p[2] for p in position_pool(game, n, K)]))
        if G >= 4:
            assert_covers_the_rules_cases(pos)
    ea, eb = make_engine(kind, game, n, K, G), make_engine(kind, game, n, K, G)
    load_one_by_one(ea, boards, hist, pos)
    res = eb.set_states(boards, hist, pos).cpu().numpy()
    assert np.all(res == _abi.SS_OK), res
    xa, xb = ea.env_step(None, want_obs=True), eb.env_step(None, want_obs=True)
    for key in ("board", "legal", "scalars", "obs"):
        assert np.array_equal(xa[key], xb[key]), key
    assert np.array_equal(xa["board"].reshape(G, -1), boards.reshape(G, -1))
    for e in (ea, eb):
        e.begin_move(None, warm_up=1)
    rounds = run_until_done([ea, eb], min_rounds=20, compare=lambda it, s: assert_same_snapshot(s[0], s[1], P=ea.P, where=(game, n, K, G, it)))
    assert rounds >= 20
    pi, cn, q, st = (t.cpu().numpy() for t in eb.read_searches())
    sa, qa = ea.status()
    for g in range(G):
        gpi, gcn, _ = ea.get_search(g, 0)
        assert pi[g].tobytes() == gpi.tobytes() and cn[g].tobytes() == gcn.tobytes(), g
    assert np.array_equal(st, sa) and q.tobytes() == qa.tobytes() and st.shape == (G, _abi.STC_COUNT) and q.shape == (G, _abi.STQ_COUNT)
    assert pi.sum() > 0 and np.all(st[:, _abi.STC_STATUS] == _abi.ST_MOVE_DONE)
    ea.close()
    eb.close()


# ---------------------------------------------------------------------------------------------------
# 2. the ACTION column
# ---------------------------------------------------------------------------------------------------
def check_actions_mixed_in_mid_search(kind, game="go", n=5, K=8, G=6):
    """One set_states with LOAD, KEEP and IDLE rows in the middle of a search: KEEP slots go on bit-identically to an undisturbed
    engine, IDLE slots report ST_IDLE, LOAD slots go on like those of a third engine with the same past that was loaded slot by slot
    (azsp_set_state) at the same moment."""
    boards, hist, pos = positions(game, n, K, G)
    dist, calm, fresh = (make_engine(kind, game, n, K, G) for _ in range(3))
    for e in (dist, calm, fresh):
        assert np.all(e.set_states(boards, hist, pos).cpu().numpy() == _abi.SS_OK)
        e.begin_move(None, warm_up=0)
    for _ in range(6):
        for e in (dist, calm, fresh):
            play_round(e, snapshot(e))
    keep, load, idle = [0, 3, 5], [1, 4], [2]
    act = np.zeros(G, dtype=np.int32)
    act[keep], act[load], act[idle] = _abi.PSA_KEEP, _abi.PSA_LOAD, _abi.PSA_IDLE
    nb, nh, npos = np.roll(boards, 2, axis=0), np.roll(hist, 2, axis=0), np.roll(pos, 2, axis=0).copy()  # slot g gets the position of slot g - 2
    npos[:, _abi.PS_ACTION] = act
    assert np.all(dist.set_states(nb, nh, npos).cpu().numpy() == _abi.SS_OK)
    load_one_by_one(fresh, nb[load], nh[load], npos[load], slots=load)
    # a loaded slot starts a new search: its begin_move state is reset, the others' must not be touched
    warm = np.full(G, _abi.BM_SKIP, dtype=np.int32)
    warm[load] = 0
    dist.begin_moves(None, warm)
    fresh.begin_move(None, warm_up=0)

    def compare(it, s):
        assert_same_snapshot(s[0], s[1], games=keep, P=dist.P, where=("keep", it))
        assert np.all(s[0][0][idle, _abi.STC_STATUS] == _abi.ST_IDLE)
        assert np.array_equal(s[0][0][load], s[2][0][load]), ("load", it)
        if it > 0:  # (the valid flags are the caller's tensor: the previous select's until the next one)
            assert not s[0][2].reshape(G, -1)[idle].any()
        rows = (np.asarray(load)[:, None] * dist.P + np.arange(dist.P)[None, :]).reshape(-1)
        assert np.array_equal(s[0][2][rows], s[2][2][rows]) and np.array_equal(s[0][3][rows[s[0][2][rows]]], s[2][3][rows[s[0][2][rows]]]), ("load", it)

    run_until_done([dist, calm, fresh], slots=keep + load, compare=compare)
    assert_same_searches(dist, calm, keep)
    assert_same_searches(dist, fresh, load)
    for e in (dist, calm, fresh):
        e.close()


def check_refused_rows(kind):
    """INVALID and GAME_OVER rows give their result code and leave the slot idle; the engine's fault flag stays clear."""
    boards, hist, pos = positions("go", 5, 8, 1)
    G, NP = 8, 25
    b, h, p = np.repeat(boards, G, axis=0), np.repeat(hist, G, axis=0), np.repeat(pos, G, axis=0).copy()
    p[:, _abi.PS_KO] = -1
    stone, empty = int(np.flatnonzero(boards[0].reshape(-1) != 0)[0]), int(np.flatnonzero(boards[0].reshape(-1) == 0)[0])
    p[0, _abi.PS_TO_PLAY] = 0          # no colour id
    p[1, _abi.PS_STEPS] = -1
    p[2, _abi.PS_CAPS_WHITE] = -3
    p[3, _abi.PS_KO] = NP              # off the board
    p[4, _abi.PS_KO] = stone           # on a stone
    p[5, _abi.PS_STEPS] = 2 * NP       # the engine's max_steps
    p[6, _abi.PS_ACTION] = 77          # no action
    p[7, _abi.PS_KO] = empty           # a ko point on an empty point is a position
    eng = make_engine(kind, "go", 5, 8, G)
    eng.reset_games()  # every slot holds a searchable game before the call
    res = eng.set_states(b, h, p).cpu().numpy()
    I, O, V = _abi.SS_INVALID, _abi.SS_OK, _abi.SS_GAME_OVER
    assert res.tolist() == [I, I, I, I, I, V, I, O], res
    eng.begin_move(None, warm_up=1)
    for _ in range(3):
        play_round(eng, snapshot(eng))  # (status() raises on an engine fault)
    st, _ = eng.status()
    assert np.all(st[:7, _abi.STC_STATUS] == _abi.ST_IDLE) and st[7, _abi.STC_STATUS] == _abi.ST_SEARCH and not eng.valid.cpu().numpy()[: 7 * eng.P].any()
    eng.close()
    boards, hist, pos = positions("gomoku", 7, 8, 1)
    b, h, p = np.repeat(boards, 3, axis=0), np.repeat(hist, 3, axis=0), np.repeat(pos, 3, axis=0).copy()
    p[0, _abi.PS_KO] = int(np.flatnonzero(boards[0].reshape(-1) == 0)[0])  # a ko point at Gomoku
    b[1] = np.where(np.indices((7, 7)).sum(axis=0) % 2 == 0, 1, 2)  # a full board
    eng = make_engine(kind, "gomoku", 7, 8, 3)
    res = eng.set_states(b, h, p).cpu().numpy()
    assert res.tolist() == [I, V, O], res
    play_round(eng, snapshot(eng))
    st, _ = eng.status()
    assert st[:, _abi.STC_STATUS].tolist() == [_abi.ST_IDLE, _abi.ST_IDLE, _abi.ST_NEED_ROOT]
    with pytest.raises(ValueError):
        eng.set_states(b, np.zeros((3, 9, 7, 7), np.int8), p)
    with pytest.raises(ValueError):
        eng.set_states(b[:2], h[:2], p[:2])
    eng.close()


# ---------------------------------------------------------------------------------------------------
# 3. begin_moves
# ---------------------------------------------------------------------------------------------------
def check_begin_moves(kind, game="go", n=5, K=8, G=4, sims=24):
    """Per-slot warm flags and noise rows: every slot's outputs equal those of a ONE-game engine given the slot's noise / flag through
    begin_move; a SKIP slot is left alone -- its noise row is not overwritten, and a search that waits for its noise goes on waiting."""
    boards, hist, pos = positions(game, n, K, G)
    pos = pos.copy()
    pos[:, _abi.PS_STEPS] = [2, 3, 30, 31]  # (below and above warm_up_steps = 16: the flag -1 derives both temperatures)
    pos[:, _abi.PS_TO_PLAY] = [1, -1, 1, -1] if game == "go" else [1, 2, 1, 2]
    pos[:, _abi.PS_KO], pos[:, _abi.PS_LAST_PASS] = -1, 0  # (no pass ends a game here: every slot keeps a sub-tree for the second move)
    rng = np.random.Generator(np.random.PCG64(5))
    A = eu.num_actions(game, n)
    na, nb, nc, nd = (rng.dirichlet(np.full(A, 0.3), size=G) for _ in range(4))
    S = _abi.BM_SKIP
    many = make_engine(kind, game, n, K, G, P=1, sims=sims, root_noise=True)
    ones = [make_engine(kind, game, n, K, 1, P=1, sims=sims, root_noise=True) for _ in range(G)]
    assert np.all(many.set_states(boards, hist, pos).cpu().numpy() == _abi.SS_OK)
    many.begin_moves(na, np.array([1, S, -1, S], dtype=np.int32))
    many.begin_moves(nb, np.array([S, 0, S, -1], dtype=np.int32))  # must not overwrite the rows of slots 0 and 2
    first = [(na[0], 1), (nb[1], 0), (na[2], -1), (nb[3], -1)]
    for g, e in enumerate(ones):
        load_one_by_one(e, boards[g:g + 1], hist[g:g + 1], pos[g:g + 1])
        e.begin_move(first[g][0], warm_up=first[g][1])
        run_until_done([e])
    run_until_done([many])
    for g, e in enumerate(ones):
        assert_same_searches(many, e, [g], [0])
    pis = many.read_searches()[0].cpu().numpy()
    assert not np.array_equal(pis[2], pis[0]) and len({p.tobytes() for p in pis}) == G
    # second move: slot 0 is skipped and goes on waiting for its noise while the others search; then it alone gets its noise
    moves = many.read_searches()[1].cpu().numpy().argmax(axis=1).astype(np.int32)
    many.commit_move(moves)
    for g, e in enumerate(ones):
        e.commit_move(moves[g:g + 1])
    st0, _ = many.status()
    assert np.all(st0[:, _abi.STC_STATUS] == _abi.ST_SEARCH), st0  # (the most visited child is a node: every slot keeps its sub-tree)
    many.begin_moves(nc, np.array([S, 1, 0, 1], dtype=np.int32))
    run_until_done([many], slots=[1, 2, 3])
    st1, _ = many.status()
    assert np.array_equal(st1[0], st0[0]) and st1[0, _abi.STC_NOISE_PENDING] == 1, (st0[0], st1[0])
    done = [t.cpu().numpy().copy() for t in many.read_searches()]
    many.begin_moves(nd, np.array([0, S, S, S], dtype=np.int32))
    run_until_done([many], slots=[0])
    after = [t.cpu().numpy() for t in many.read_searches()]
    assert all(np.array_equal(x[1:], y[1:]) for x, y in zip(done, after))  # the finished slots were left alone
    second = [(nd[0], 0), (nc[1], 1), (nc[2], 0), (nc[3], 1)]
    for g, e in enumerate(ones):
        e.begin_move(second[g][0], warm_up=second[g][1])
        run_until_done([e])
        assert_same_searches(many, e, [g], [0])
        e.close()
    many.close()


# ---------------------------------------------------------------------------------------------------
# 4. pinned to the reference: all games of a golden file at once through uct_search_many
# ---------------------------------------------------------------------------------------------------
def check_golden_games_at_once(kind, name, max_moves=None, device_route=False):
    """check_dropin_search's replay for ALL games of a golden file simultaneously: slot i holds game i, the recorded noise and uniforms
    are served per env in the documented order (one dirichlet per env in list order, then the choice draws of env 0, env 1, ...),
    sub-tree reuse goes through the batch handle, games end at different plies and leave the batch, and a slot without a reusable
    sub-tree is loaded again.  Moves, pi, root Q and child Q equal the golden records, and the handle's has_next equals the golden's
    has_next.  The reference hands out the chosen child also when it is the terminal position of the move that ends the game; the
    engine keeps no terminal sub-tree, so `reusable` equals has_next on every move but a game's last, where it must be False."""
    from alpha_zero_amd.core.mcts_v2 import parallel_uct_search_many, uct_search_many

    G = golden_mcts.MctsGolden(name)
    g, cfg = G.g, G.cfg
    ng = cfg["games"]
    envs = [dc.make_env(kind, cfg["game"], cfg["n"]) for _ in range(ng)]
    ef = make_eval_func(G.A)
    if device_route:
        from arena_checks import SynthDeviceEvaluator

        ef = SynthDeviceEvaluator(G.A, 2.0)
    idx = [G.moves_of_game(gi)[:max_moves] for gi in range(ng)]
    ply = [0] * ng
    real_dir, real_choice = np.random.dirichlet, np.random.choice
    handle, steps, reloads = None, 0, 0
    try:
        while True:
            live = [gi for gi in range(ng) if ply[gi] < len(idx[gi]) and not envs[gi].is_game_over()]
            if not live:
                break
            recs = [int(idx[gi][ply[gi]]) for gi in live]
            noises = [g["noise"][i] for i in recs]
            us = [u for i in recs for u in g["uniforms"][i][: g["n_uniforms"][i]]]
            np.random.dirichlet = lambda alphas, _q=noises: _q.pop(0)

            def choice(a, p=None, _us=us):
                cdf = np.asarray(p, dtype=np.float64).cumsum()
                cdf /= cdf[-1]
                return a[cdf.searchsorted(_us.pop(0), side="right")]

            np.random.choice = choice
            kw = dict(envs=[envs[gi] for gi in live], eval_func=ef, root_nodes=handle if cfg.get("reuse", True) else None,
                      c_puct_base=cfg["c_puct_base"], c_puct_init=cfg["c_puct_init"], num_simulations=cfg["sims"], root_noise=cfg.get("root_noise", True),
                      warm_up=[bool(g["warm_up"][i]) for i in recs], deterministic=cfg.get("deterministic", False))
            if cfg["parallel"] > 1:
                moves, pis, rqs, cqs, handle = parallel_uct_search_many(num_parallel=cfg["parallel"], **kw)
            else:
                moves, pis, rqs, cqs, handle = uct_search_many(**kw)
            assert not us and (not noises or not cfg.get("root_noise", True)), (name, steps)
            for k, (gi, i) in enumerate(zip(live, recs)):
                where = (name, gi, ply[gi])
                assert moves[k] == g["move"][i], where
                assert str(pis[k].dtype) == str(g["pi_dtype"][i])
                if cfg["game"] == "go":
                    assert np.array_equal(pis[k], g["pi"][i]), where
                else:
                    assert np.abs(pis[k] - g["pi"][i]).max() <= 1e-6, where
                assert rqs[k] == g["root_q"][i] and cqs[k] == g["child_q"][i], where
                assert handle.has_next(envs[gi]) == bool(g["has_next"][i]), where
                envs[gi].step(int(moves[k]))
                assert handle.reusable(envs[gi]) == (bool(g["has_next"][i]) and not envs[gi].is_game_over()), where
                reloads += not handle.reusable(envs[gi])
                ply[gi] += 1
            steps += 1
    finally:
        np.random.dirichlet, np.random.choice = real_dir, real_choice
    assert steps > 0 and all(p > 0 for p in ply)
    if device_route:
        assert ef.calls > 0
    return dict(steps=steps, plies=ply, reloads=reloads)


# ---------------------------------------------------------------------------------------------------
# 6. errors
# ---------------------------------------------------------------------------------------------------
def check_errors(kind):
    from alpha_zero_amd.core.mcts_v2 import uct_search_many

    ef = make_eval_func(26)
    go5 = [dc.make_env(kind, "go", 5) for _ in range(2)]
    args = (ef, None, 19652.0, 1.25, 8)
    with pytest.raises(ValueError):
        uct_search_many([go5[0], object()], *args)
    with pytest.raises(ValueError):
        uct_search_many(go5, ef, None, 19652.0, 1.25, 0)
    for other in (dc.make_env(kind, "go", 9), dc.make_env(kind, "gomoku", 7), dc.make_env(kind, "go", 5, komi=5.5), dc.make_env(kind, "go", 5, num_stack=4)):
        with pytest.raises(ValueError, match="share"):
            uct_search_many([go5[0], other], *args)
    with pytest.raises(ValueError, match="share"):
        uct_search_many([dc.make_env(kind, "gomoku", 7), dc.make_env(kind, "gomoku", 7, num_to_win=4)], make_eval_func(49), None, 19652.0, 1.25, 8)

    class Wrong:  # an evaluator that names its network's input planes (core/evaluate.py DeviceEvaluator does)
        in_channels = 9

        def __call__(self, obs, batched=False):
            raise AssertionError("must not be called")

    with pytest.raises(ValueError, match="input planes"):
        uct_search_many(go5, Wrong(), None, 19652.0, 1.25, 8)
    bs = BatchSearch.for_env(go5[0], 2, 8)
    with pytest.raises(ValueError, match="input planes"):
        bs.load_envs(go5)
        bs.search(Wrong())
    with pytest.raises(ValueError, match="do not fit"):
        bs.load_envs(go5 + [dc.make_env(kind, "go", 5)])
    with pytest.raises(ValueError, match="share"):
        bs.load_envs([dc.make_env(kind, "go", 5, komi=0.5)])
    bs.close()
    # a handle is checked against its envs: stepping an env by another move than the one returned, or handing in foreign objects
    moves, _, _, _, handle = uct_search_many(go5, ef, None, 19652.0, 1.25, 16, deterministic=True)
    assert handle.reusable(go5[0]) and handle.reusable(go5[1])
    go5[0].step(int(moves[0]))
    go5[1].step(int(np.flatnonzero(go5[1].legal_actions[:25] * (np.arange(25) != moves[1]))[0]))
    with pytest.raises(ValueError, match="does not belong"):
        uct_search_many(go5, ef, handle, 19652.0, 1.25, 16)
    with pytest.raises(ValueError, match="handle"):
        uct_search_many(go5, ef, object(), 19652.0, 1.25, 16)
    moves, _, _, _, handle = uct_search_many(go5, ef, None, 19652.0, 1.25, 16, deterministic=True)
    with pytest.raises(ValueError, match="handle"):
        uct_search_many(go5, ef, handle, 19652.0, 1.25, 17)  # other settings than the handle's
    with pytest.raises(ValueError, match="do not fit"):
        uct_search_many(go5 + [dc.make_env(kind, "go", 5)], ef, handle, 19652.0, 1.25, 16)
    go5[0].step(25)
    go5[0].step(25)
    with pytest.raises(RuntimeError, match="Game is over"):
        uct_search_many(go5, ef, None, 19652.0, 1.25, 8)


def check_batch_search_object(kind):
    """BatchSearch used directly: tensors in, device tensors out; per-position warm flags; commit reports the slots that kept a tree,
    and a reloaded slot joins the kept ones in the next search.  Every slot equals a one-game engine on its position alone."""
    n, sims = 5, 24
    boards, hist, pos = (x[[0, 2, 3]] for x in positions("go", n, 8, 4))  # (not the one after a pass: a second pass would end its game)
    ef = make_eval_func(26)
    env0 = dc.make_env(kind, "go", n)
    bs = BatchSearch.for_env(env0, 4, sims)
    dev = bs.eng.device
    res = bs.load(torch.from_numpy(boards).to(dev), torch.from_numpy(hist).to(dev), torch.from_numpy(pos).to(dev), slots=[3, 0, 2])
    assert res.tolist() == [0, 0, 0] and bs.slots.tolist() == [0, 2, 3]
    bs.search(ef, warm_up=[False, True, False])
    out = bs.results()
    assert out.pi.device.type == dev.type and out.pi.dtype == torch.float64 and out.pi.shape == (3, 26) and out.child_N.dtype == torch.float32
    pi, cn, rq = out.cpu()
    moves = cn.argmax(axis=1)
    cq, reusable = bs.commit(moves)
    for row, (i, warm) in enumerate(((1, False), (2, True), (0, False))):  # slot 0 holds position 1, slot 2 position 2, slot 3 position 0
        one = make_engine(kind, "go", n, 8, 1, P=1, sims=sims)
        load_one_by_one(one, boards[i:i + 1], hist[i:i + 1], pos[i:i + 1])
        one.begin_move(None, warm_up=int(warm))
        run_until_done([one])
        gpi, gcn, _ = one.get_search(0, 0)
        assert gpi.tobytes() == pi[row].tobytes() and gcn.tobytes() == cn[row].tobytes()
        one.commit_move(moves[row:row + 1].astype(np.int32))
        st, q = one.status()
        assert q[0, _abi.STQ_ROOT_Q] == rq[row] and q[0, _abi.STQ_CHILD_Q] == cq[row] and (st[0, _abi.STC_STATUS] == _abi.ST_SEARCH) == reusable[row]
        one.close()
    assert reusable.all() and bs.slots.tolist() == [0, 2, 3]
    # keep slots 0 and 3, drop slot 2, load a new position into slot 1
    bs.load(boards[:1], hist[:1], pos[:1], slots=[1], keep=[0, 3])
    assert bs.slots.tolist() == [0, 1, 3]
    bs.search(ef)
    st, _ = bs.eng.status()
    assert st[:, _abi.STC_STATUS].tolist() == [_abi.ST_MOVE_DONE, _abi.ST_MOVE_DONE, _abi.ST_IDLE, _abi.ST_MOVE_DONE]
    assert bs.results().pi.shape == (3, 26)
    bs.close()


# ---------------------------------------------------------------------------------------------------
# 5. batch == sequential with the product evaluator (device only)
# ---------------------------------------------------------------------------------------------------
def check_batch_equals_sequential_with_product_evaluator(name="gomoku13_ckpt200000_p1_s100", plies=(1, 3, 5, 8)):
    """Four positions from different plies of a golden game, searched at once (uct_search_many) and then one by one (uct_search) with
    the SAME DeviceEvaluator around the shipped Gomoku checkpoint on the fp32-class kernels: moves, pi, root Q and child Q are
    bit-identical, and the evaluator's range record counts no event.  This rests on the documented batch independence of the
    evaluator kernels (a row's outputs do not depend on the batch it arrives in)."""
    import realnet_checks as rc
    from alpha_zero_amd import _lib
    from alpha_zero_amd.core.evaluate import DeviceEvaluator
    from alpha_zero_amd.core.mcts_v2 import uct_search, uct_search_many
    from alpha_zero_amd.core.network import InferenceNet, widen_network

    G = golden_mcts.MctsGolden(name)
    g, cfg = G.g, G.cfg
    idx = G.moves_of_game(0)
    envs = []
    for k in plies:
        env = dc.make_env("gpu", cfg["game"], cfg["n"])
        for i in idx[:k]:
            env.step(int(g["move"][i]))
        assert not env.is_game_over() and env.steps == k
        envs.append(env)
    recs = [int(idx[k]) for k in plies]
    inf = InferenceNet(widen_network(rc.load_shipped(), 64), dtype=torch.float32, binding=_lib.load()).cuda()
    assert "split-precision" in inf.evaluator_path(cfg["n"], "cuda")
    ev = DeviceEvaluator(inf)
    kw = dict(c_puct_base=cfg["c_puct_base"], c_puct_init=cfg["c_puct_init"], num_simulations=cfg["sims"], root_noise=True)
    real_dir, real_choice = np.random.dirichlet, np.random.choice

    def serve(records):  # the recorded Dirichlet draws, and one recorded uniform per search: a Gomoku pi has no mass on an illegal move
        noises, us = [g["noise"][i] for i in records], [float(g["uniforms"][i][0]) for i in records]
        np.random.dirichlet = lambda alphas: noises.pop(0)

        def choice(a, p=None):
            cdf = np.asarray(p, dtype=np.float64).cumsum()
            cdf /= cdf[-1]
            return a[cdf.searchsorted(us.pop(0), side="right")]

        np.random.choice = choice
        return noises, us

    try:
        seq = []
        for env, i in zip(envs, recs):
            left = serve([i])
            seq.append(uct_search(env, ev, None, warm_up=bool(g["warm_up"][i]), **kw)[:4])
            assert not left[0] and not left[1]
        left = serve(recs)
        many_moves, many_pi, many_rq, many_cq, _ = uct_search_many(envs, ev, None, warm_up=[bool(g["warm_up"][i]) for i in recs], **kw)
        assert not left[0] and not left[1]
    finally:
        np.random.dirichlet, np.random.choice = real_dir, real_choice
    for k, (move, pi, rq, cq) in enumerate(seq):
        print("ply", plies[k], "sequential", int(move), rq, cq, "batched", int(many_moves[k]), many_rq[k], many_cq[k], "max |dpi|", float(np.abs(pi - many_pi[k]).max()))
    for k, (move, pi, rq, cq) in enumerate(seq):
        assert move == many_moves[k] and pi.dtype == many_pi[k].dtype and pi.tobytes() == many_pi[k].tobytes(), (plies[k], move, many_moves[k])
        assert rq == many_rq[k] and cq == many_cq[k], (plies[k], rq, many_rq[k], cq, many_cq[k])
    assert inf._split is not None and inf.split_range_status(reset=True)[0] == 0
