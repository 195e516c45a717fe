"""Shared drivers of the auxiliary training targets (azsp_set_aux_targets / azsp_harvest_aux / azsp_replay_gather_aux:
EngineConfig.aux_targets, Engine.harvest(with_aux=True), SelfPlayActor(aux_targets=True), DeviceReplay(aux_targets=True)).  The same
functions run on the host twin (CPU tier) and on the device (`-m gpu`).

The yardstick is restated here, not taken from the engine: the final board of a game is the replay of its harvested moves through the
CPU oracle's env, its ownership a NumPy flood fill of Tromp-Taylor's rule (a stone belongs to its colour, an empty region to a colour
iff it borders that colour only, anything else to nobody), the root value the logged AZSP_SQ_ROOT_Q, the dihedral maps those of
symmetry_checks.  Every comparison is exact."""
import numpy as np
import pytest
import torch

import engine_util as eu
from alpha_zero_amd import _abi
from alpha_zero_amd.core.engine import Engine, EngineConfig
from alpha_zero_amd.core.replay import DeviceReplay
from budget_checks import SynthActor
from symmetry_checks import d_planes, d_policy
from synth_eval import eval_batch

G, P, KOMI, EINVAL = 8, 2, 7.5, -1


# ---------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------
def tromp_taylor_owner(board):
    """board int[n, n], +1 black / -1 white / 0 empty -> int8[n, n]: +1 / -1 the point counts for black / white, 0 for nobody."""
    n = board.shape[0]
    own = np.array(board, dtype=np.int8)
    seen = board != 0
    for i0 in range(n):
        for j0 in range(n):
            if seen[i0, j0]:
                continue
            region, borders, stack = [], set(), [(i0, j0)]
            seen[i0, j0] = True
            while stack:
                i, j = stack.pop()
                region.append((i, j))
                for a, b in ((i - 1, j), (i + 1, j), (i, j - 1), (i, j + 1)):
                    if not (0 <= a < n and 0 <= b < n):
                        continue
                    if board[a, b] != 0:
                        borders.add(int(board[a, b]))
                    elif not seen[a, b]:
                        seen[a, b] = True
                        stack.append((a, b))
            if len(borders) == 1:
                colour = next(iter(borders))
                for i, j in region:
                    own[i, j] = colour
    return own


def check_restatement():
    """The flood fill on boards whose ownership is known by inspection: a mistake in this file's own yardstick would otherwise go
    unnoticed wherever the engine made the same one."""
    b = np.zeros((5, 5), np.int8)
    assert not tromp_taylor_owner(b).any()  # an empty board borders nobody
    b[:, 2] = 1  # a black wall: both sides touch black only
    assert (tromp_taylor_owner(b) == 1).all()
    b[2, 4] = -1  # a white stone on the right: that side is nobody's, the left stays black's
    want = np.zeros((5, 5), np.int8)
    want[:, :3], want[2, 4] = 1, -1
    assert np.array_equal(tromp_taylor_owner(b), want)
    b = np.array([[0, -1, 0, 1, 0], [-1, -1, 0, 1, 1], [0, 0, 0, 0, 0], [1, 1, 0, -1, -1], [0, 1, 0, -1, 0]], np.int8)
    want = b.copy()
    want[0, 0], want[0, 4], want[4, 0], want[4, 4] = -1, 1, 1, -1  # four one-point eyes, a neutral cross
    assert np.array_equal(tromp_taylor_owner(b), want)


def final_board(game, n, moves, max_steps=0, num_to_win=5):
    """The board after `moves` (a game's harvested moves; a resignation, -1, is no board move) replayed through the CPU oracle's env, in
    black +1 / white -1 whatever the game's own colour ids."""
    env = eu.make_oracle_env(game, n, max_steps, num_to_win)
    env.reset()
    for m in moves:
        if m >= 0:
            env.step(int(m))
    b = env.board.astype(np.int8)
    return np.where(b == env.black_player, 1, np.where(b == env.white_player, -1, 0)).astype(np.int8)


# ---------------------------------------------------------------------------------------------------
# engines that play by themselves on the synthetic evaluator
# ---------------------------------------------------------------------------------------------------
def make_engine(kind, game="go", n=5, aux=True, sims=8, seed=7, num_games=G, **kw):
    b, dev = eu.backend(kind)
    kw.setdefault("stop_at_game_end", True)
    eng = Engine(b, EngineConfig(game=game, board_size=n, num_games=num_games, num_parallel=P, num_simulations=sims, warm_up_steps=4, komi=KOMI,
                                 seed=seed, aux_targets=aux, **kw), device=dev)
    eng.reset_games()
    return eng


def play(eng, done=_abi.ST_IDLE, limit=20000):
    """select -> synthetic evaluator on the valid rows -> round, until every slot's status is `done`."""
    eng.select()
    for _ in range(limit):
        valid = eng.valid.cpu().numpy().astype(bool)
        if not valid.any() and np.all(eng.status()[0][:, _abi.STC_STATUS] == done):
            return
        rows = np.flatnonzero(valid)
        pri, val = np.zeros((eng.rows, eng.A), np.float32), np.zeros(eng.rows, np.float32)
        if len(rows):
            pri[rows], val[rows] = eval_batch(eu.decode_features(eng)[rows], eng.A)
        eng.priors.copy_(torch.from_numpy(pri))
        eng.values.copy_(torch.from_numpy(val))
        eng.round()
    raise AssertionError("the games did not finish")


def drain(eng, with_aux=True, **kw):
    """Every finished game: dict of host arrays (states, pi, z, games with START rebased, moves[, ownership, score, root_q])."""
    keys = ("states", "pi", "z", "games", "moves") + (("ownership", "score", "root_q") if with_aux else ())
    parts, base = [], 0
    while True:
        got = eng.harvest(with_moves=True, with_aux=with_aux, **kw)
        if len(got[3]) == 0:
            break
        games = got[3].copy()
        games[:, _abi.GR_START] += base
        base += len(got[2])
        parts.append([t.cpu().numpy().copy() if i != 3 else games for i, t in enumerate(got)])
    assert parts
    out = {k: np.concatenate([p[i] for p in parts]) for i, k in enumerate(keys)}
    if with_aux:
        nn = len(out["z"])
        assert out["ownership"].dtype == np.int8 and out["ownership"].shape == (nn, eng.N, eng.N)
        assert out["score"].dtype == out["root_q"].dtype == np.float32 and out["score"].shape == out["root_q"].shape == (nn,)
    return out


def mover_sign(states):
    """+1 for a sample whose mover is black, -1 for white: the colour plane, the last one."""
    return np.where(states[:, -1, 0, 0] == 1, 1, -1)


def assert_go_game(h, row, n, max_steps):
    """Ownership and score of every sample of Go game `row` equal mover-sign x the restatement on the replayed final board; returns
    black's ownership map."""
    st, mv, own, sc = eu.samples_of(row, h["states"], h["moves"], h["ownership"], h["score"])
    want = tromp_taylor_owner(final_board("go", n, mv, max_steps))
    cb, cw = int((want == 1).sum()), int((want == -1).sum())
    for k, s in enumerate(mover_sign(st)):
        where = (int(row[_abi.GR_SLOT]), int(row[_abi.GR_UID]), k)
        assert np.array_equal(own[k], s * want), where
        assert sc[k].tobytes() == np.float32(s * (cb - (cw + KOMI))).tobytes(), where
    resigned = int(row[_abi.GR_RESIGNED])
    assert (mv[-1] == -1) == bool(resigned) and np.all(mv[:-1] >= 0)
    if resigned:
        assert row[_abi.GR_AREA_BLACK] == 0 and row[_abi.GR_AREA_WHITE] == 0  # as they always were for a resigned game
    else:
        assert int(want.sum()) == int(row[_abi.GR_AREA_BLACK]) - int(row[_abi.GR_AREA_WHITE])
        assert (cb, cw) == (int(row[_abi.GR_AREA_BLACK]), int(row[_abi.GR_AREA_WHITE]))
    return want


# ---------------------------------------------------------------------------------------------------
# 1. ownership and score, Go
# ---------------------------------------------------------------------------------------------------
GO_SHAPES = {5: dict(max_steps=24, seed=7), 9: dict(max_steps=30, seed=7), 19: dict(max_steps=12, seed=7)}


def check_go_ownership_and_score(kind, n):
    """Boards of 1, 2 and 6 words.  Every sample's ownership row is mover-sign x the restatement, its score float32(s (cb - (cw + komi)));
    for a game ended by score the ownership sums to AREA_BLACK - AREA_WHITE.  The harvest holds a game ended by score and a row
    with all of -1, 0 and +1."""
    s = GO_SHAPES[n]
    eng = make_engine(kind, "go", n, max_steps=s["max_steps"], seed=s["seed"])
    play(eng)
    h = drain(eng)
    eng.close()
    assert len(h["games"]) == G
    for row in h["games"]:
        assert_go_game(h, row, n, s["max_steps"])
    assert np.any(h["games"][:, _abi.GR_RESIGNED] == 0)
    assert any({-1, 0, 1} <= set(np.unique(o).tolist()) for o in h["ownership"])
    assert len(set(mover_sign(h["states"]).tolist())) == 2 and np.any(h["score"] > 0) and np.any(h["score"] < 0)


# ---------------------------------------------------------------------------------------------------
# 2. resignation
# ---------------------------------------------------------------------------------------------------
def check_resignation(kind, n=5, max_steps=24, after=6):
    """A threshold no root value can reach (2.0) makes every game that may resign do so at the first move past `after` steps: its
    ownership and score are those of the board at the resignation, its AREA columns stay 0."""
    eng = make_engine(kind, "go", n, max_steps=max_steps, resign_threshold=2.0, check_resign_after_steps=after, force_resign_disabled=0)
    play(eng)
    h = drain(eng)
    eng.close()
    resigned = h["games"][h["games"][:, _abi.GR_RESIGNED] == 1]
    assert len(resigned) >= 1
    for row in h["games"]:
        want = assert_go_game(h, row, n, max_steps)
        if row[_abi.GR_RESIGNED]:
            assert int(row[_abi.GR_LENGTH]) == after + 2  # steps 0..after are played, the move at step after + 1 resigns
            assert np.any(want == 1) and np.any(want == -1)  # a board with stones: the target is not the empty map


# ---------------------------------------------------------------------------------------------------
# 3. root value
# ---------------------------------------------------------------------------------------------------
def check_root_value(kind, reuse_tree, n=5, max_steps=14):
    """root_q of sample k of a slot's game is the logged AZSP_SQ_ROOT_Q of its ply k as float32, bit for bit."""
    eng = make_engine(kind, "go", n, max_steps=max_steps, reuse_tree=bool(reuse_tree), log_moves=True, log_capacity=max_steps)
    play(eng)
    logged = {(g, k): eng.get_search(g, k)[2][_abi.SQ_ROOT_Q] for g in range(G) for k in range(max_steps)}
    h = drain(eng)
    eng.close()
    assert len(h["games"]) == G
    seen = []
    for row in h["games"]:
        rq = eu.samples_of(row, h["root_q"])
        for k in range(len(rq)):
            want = np.float32(logged[(int(row[_abi.GR_SLOT]), k)])
            assert rq[k].tobytes() == want.tobytes(), (int(row[_abi.GR_SLOT]), k, rq[k], want)
            seen.append(float(want))
    assert len(set(seen)) > len(seen) // 2 and np.any(np.array(seen) != 0)  # (not a column of one constant)
    # the double the log holds is not always a float32: the staged value is its rounding, not a copy that happens to fit
    assert any(float(np.float32(v)) != v for v in logged.values())


# ---------------------------------------------------------------------------------------------------
# 4. both staging buffers
# ---------------------------------------------------------------------------------------------------
def check_both_staging_buffers(kind, n=5, max_steps=6):
    """Without a harvest every slot fills both of its staging buffers and stalls; one harvest then hands out two games per slot, each
    with the ownership of its own final board."""
    eng = make_engine(kind, "go", n, max_steps=max_steps, stop_at_game_end=False)
    play(eng, done=_abi.ST_WAIT_BUF)
    h = drain(eng, sample_capacity=2 * G * max_steps, max_games=2 * G)
    eng.close()
    assert len(h["games"]) == 2 * G
    maps = {}
    for row in h["games"]:
        maps.setdefault(int(row[_abi.GR_SLOT]), []).append(assert_go_game(h, row, n, max_steps))
    assert sorted(maps) == list(range(G)) and all(len(v) == 2 for v in maps.values())
    assert any(not np.array_equal(a, b) for a, b in maps.values())  # the two buffers of a slot hold different maps: none leaked into the other


# ---------------------------------------------------------------------------------------------------
# 5. nothing else moves
# ---------------------------------------------------------------------------------------------------
def check_nothing_else_moves(kind, n=5, max_steps=14):
    """Same seed with and without aux targets: states, pi, z, game rows, moves and counters are identical.  The refusals of the two
    calls; each of the three harvest outputs alone."""
    b, dev = eu.backend(kind)
    on, off = (make_engine(kind, "go", n, aux=a, max_steps=max_steps) for a in (True, False))
    assert b.dll.azsp_harvest_aux(off.h, None, None, None) == 0
    buf = torch.zeros(4 * G * max_steps * n * n, dtype=torch.float32, device=dev)
    for args in ((buf.data_ptr(), None, None), (None, buf.data_ptr(), None), (None, None, buf.data_ptr())):
        assert b.dll.azsp_harvest_aux(off.h, *args) == EINVAL  # never enabled: nothing is staged
    with pytest.raises(_abi.AzspError):
        off.harvest(with_aux=True)
    play(on), play(off)
    assert on.counters() == off.counters()
    hon, hoff = drain(on), drain(off, with_aux=False)
    for key in ("states", "pi", "z", "games", "moves"):
        assert hon[key].tobytes() == hoff[key].tobytes() and hon[key].shape == hoff[key].shape, key
    on.close(), off.close()
    # a drop-in engine records no samples
    drop = Engine(b, EngineConfig(game="go", board_size=n, num_games=2, num_parallel=1, num_simulations=4, stop_after_move=True), device=dev)
    assert b.dll.azsp_set_aux_targets(drop.h, 1) == EINVAL and b.dll.azsp_set_aux_targets(drop.h, 0) == EINVAL
    drop.close()
    with pytest.raises(_abi.AzspError):
        Engine(b, EngineConfig(game="go", board_size=n, num_games=2, num_parallel=1, num_simulations=4, stop_after_move=True, aux_targets=True), device=dev)
    # one output at a time, two games per harvest; the games are found again by their slot
    by_slot = {int(r[_abi.GR_SLOT]): {k: eu.samples_of(r, hon[k]) for k in ("ownership", "score", "root_q")} for r in hon["games"]}
    eng = make_engine(kind, "go", n, max_steps=max_steps)
    play(eng)
    cap = 2 * max_steps
    outs = dict(ownership=torch.full((cap, n, n), 77, dtype=torch.int8, device=dev), score=torch.full((cap,), 77.0, dtype=torch.float32, device=dev),
                root_q=torch.full((cap,), 77.0, dtype=torch.float32, device=dev))
    for only in ("ownership", "score", "root_q", None):
        for t in outs.values():
            t.fill_(77)
        assert b.dll.azsp_harvest_aux(eng.h, *[t.data_ptr() if k == only else None for k, t in outs.items()]) == 0
        games = eng.harvest(sample_capacity=cap, max_games=2)[3]  # (a harvest without with_aux leaves the pointers set above alone)
        assert len(games) == 2
        for row in games:
            for k, t in outs.items():
                got = eu.samples_of(row, t.cpu().numpy())
                if k == only:
                    assert got.tobytes() == by_slot[int(row[_abi.GR_SLOT])][k].tobytes(), (only, k)
                else:
                    assert np.all(got == 77), (only, k)
    eng.close()


# ---------------------------------------------------------------------------------------------------
# 6. Gomoku
# ---------------------------------------------------------------------------------------------------
def check_gomoku(kind, n=7, num_to_win=4):
    """Ownership is mover-sign x (black stones - white stones) of the final board, score is z."""
    eng = make_engine(kind, "gomoku", n, num_to_win=num_to_win)
    play(eng)
    h = drain(eng)
    eng.close()
    assert len(h["games"]) == G
    for row in h["games"]:
        st, mv, own, sc, z = eu.samples_of(row, h["states"], h["moves"], h["ownership"], h["score"], h["z"])
        want = final_board("gomoku", n, mv, num_to_win=num_to_win)
        assert int((want != 0).sum()) == len(mv)
        for k, s in enumerate(mover_sign(st)):
            assert np.array_equal(own[k], s * want), (int(row[_abi.GR_SLOT]), k)
        assert sc.tobytes() == z.tobytes()
    assert np.any(h["score"] == 1) and np.any(h["score"] == -1)


# ---------------------------------------------------------------------------------------------------
# 7. replay
# ---------------------------------------------------------------------------------------------------
def _samples(rng, n, A, count, dev):
    return dict(states=torch.from_numpy(rng.integers(0, 2, size=(count, 17, n, n)).astype(np.int8)).to(dev),
                pi=torch.from_numpy(rng.random((count, A)).astype(np.float32)).to(dev),
                z=torch.from_numpy(rng.choice([-1.0, 0.0, 1.0], size=count).astype(np.float32)).to(dev),
                ownership=torch.from_numpy(rng.integers(-1, 2, size=(count, n, n)).astype(np.int8)).to(dev),
                score=torch.from_numpy((rng.integers(-60, 60, size=count) + 0.5).astype(np.float32)).to(dev),
                root_q=torch.from_numpy(rng.uniform(-1, 1, size=count).astype(np.float32)).to(dev))


def _aux(s, keep=None):
    return tuple(s[k] if keep is None else s[k][keep] for k in ("ownership", "score", "root_q"))


def check_replay(kind, n):
    """A ring filled past its capacity: for all 8 ops sample_device(with_aux=True) returns the ownership rows of the drawn indices
    under the NumPy D_op, score and root_q as stored, and states, pi, z as azsp_replay_gather returns them.  keep= filters aux with
    the samples; get_state -> set_state carries the rings, a state without the "aux" key loads zero rings."""
    b, dev = eu.backend(kind)
    A, cap, count, B = n * n + 1, 37, 23, 19
    rng = np.random.Generator(np.random.PCG64(3 + n))
    rep = DeviceReplay(cap, np.random.RandomState(1), n, A, device=dev, binding=b, aux_targets=True)
    first, second = _samples(rng, n, A, count, dev), _samples(rng, n, A, count, dev)
    games = np.zeros((3, _abi.GR_COUNT), dtype=np.int32)
    with pytest.raises(ValueError, match="aux"):
        rep.add_harvest(first["states"], first["pi"], first["z"], games)  # required by a replay with the rings
    with pytest.raises(ValueError, match="aux"):
        rep.add_samples(first["states"], first["pi"], first["z"], aux=_aux(first)[:2])
    rep.add_harvest(first["states"], first["pi"], first["z"], games, aux=_aux(first))
    keep = torch.from_numpy(rng.random(count) < 0.8).to(dev)
    k = keep.cpu().numpy()
    m = int(k.sum())
    assert count + m > cap and m < count  # the second insert wraps, and the mask drops something
    rep.add_harvest(second["states"], second["pi"], second["z"], games, keep=keep, aux=_aux(second))
    assert (rep.num_samples_added, rep.num_games_added, rep.size) == (count + m, 6, cap)
    # the ring as the reference's per-transition loop leaves it, restated on the host
    want = {key: np.zeros((cap,) + tuple(first[key].shape[1:]), dtype=first[key].cpu().numpy().dtype) for key in first}
    stream = {key: np.concatenate([first[key].cpu().numpy(), second[key].cpu().numpy()[k]]) for key in first}
    for i in range(count + m):
        for key in want:
            want[key][i % cap] = stream[key][i]
    for key, ring in (("states", rep.states), ("pi", rep.pi), ("z", rep.z), ("ownership", rep.ownership), ("score", rep.score), ("root_q", rep.root_q)):
        assert np.array_equal(ring.cpu().numpy(), want[key]), key
    for op in range(8):
        rep.random_state = np.random.RandomState(10 + op)
        idx = np.random.RandomState(10 + op).randint(low=0, high=cap, size=B)
        st, pi, z, own, sc, rq = (t.cpu().numpy() for t in rep.sample_device(B, transform=op, with_aux=True))
        assert own.dtype == np.float32 and np.array_equal(own, d_planes(want["ownership"][idx], op).astype(np.float32)), op
        assert sc.tobytes() == want["score"][idx].tobytes() and rq.tobytes() == want["root_q"][idx].tobytes(), op
        pst, ppi, pz = (t.cpu().numpy() for t in rep._gather(idx, op, torch.float32))  # azsp_replay_gather on the same indices
        assert st.tobytes() == pst.tobytes() and pi.tobytes() == ppi.tobytes() and z.tobytes() == pz.tobytes(), op
        assert np.array_equal(st, d_planes(want["states"][idx], op).astype(np.float32)) and np.array_equal(pi, d_policy(want["pi"][idx], op, n)), op
        if op in (3, 5):  # (a quarter turn is not its inverse: the ownership turned the wrong way would differ)
            assert not np.array_equal(own, d_planes(want["ownership"][idx], 8 - op).astype(np.float32))
    rep.random_state = np.random.RandomState(5)
    plain = rep.sample_device(B, transform=3)
    assert len(plain) == 3  # without with_aux: what it always returned
    state = rep.get_state()
    assert set(state) == {"num_games_added", "num_samples_added", "storage", "aux"}
    back = DeviceReplay(cap, np.random.RandomState(1), n, A, device=dev, binding=b, aux_targets=True)
    back.set_state(state)
    for a, c in ((rep.states, back.states), (rep.z, back.z), (rep.ownership, back.ownership), (rep.score, back.score), (rep.root_q, back.root_q)):
        assert np.array_equal(a.cpu().numpy(), c.cpu().numpy())
    assert (back.num_samples_added, back.num_games_added) == (rep.num_samples_added, rep.num_games_added)
    del state["aux"]
    back.set_state(state)
    assert not back.ownership.any() and not back.score.any() and not back.root_q.any() and np.array_equal(back.z.cpu().numpy(), rep.z.cpu().numpy())
    noaux = DeviceReplay(cap, np.random.RandomState(1), n, A, device=dev, binding=b)
    with pytest.raises(ValueError, match="aux"):
        noaux.add_samples(first["states"], first["pi"], first["z"], aux=_aux(first))
    noaux.add_samples(first["states"], first["pi"], first["z"])
    assert set(noaux.get_state()) == {"num_games_added", "num_samples_added", "storage"}
    with pytest.raises(ValueError, match="aux"):
        noaux.sample_device(4, with_aux=True)
    # the C entry refuses a ring without its output
    idx = torch.zeros(1, dtype=torch.int64, device=dev)
    o = [torch.zeros(17 * n * n, dtype=torch.float32, device=dev) for _ in range(3)]
    rc = b.dll.azsp_replay_gather_aux(rep.states.data_ptr(), rep.pi.data_ptr(), rep.z.data_ptr(), idx.data_ptr(), 1, 17, n, A, 0, _abi.FEAT_F32,
                                      o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), rep.ownership.data_ptr(), None, None, None, None, None, None)
    assert rc == EINVAL


# ---------------------------------------------------------------------------------------------------
# 8. the actor
# ---------------------------------------------------------------------------------------------------
def _actor(kind, n=5, max_steps=12, **kw):
    import warnings

    from alpha_zero_amd.core.network import AlphaZeroNet

    b, dev = eu.backend(kind)
    ekw = dict(stop_at_game_end=True, max_steps=max_steps)
    ekw.update(kw.pop("engine_kw", {}))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # (the tiny network has no hand-written kernels; its forward is never run)
        return SynthActor(AlphaZeroNet((17, n, n), n * n + 1, 1, 8, 8), game="go", board_size=n, num_games=G, num_simulations=8, num_parallel=P,
                          warm_up_steps=4, seed=7, device=dev, net_dtype=torch.float32, use_graph=False, binding=b, tiled_features=False,
                          engine_kw=ekw, **kw)


def _finish(actor):
    for _ in range(400):
        actor.run_rounds(8)
        if np.all(actor.engine.status()[0][:, _abi.STC_STATUS] == _abi.ST_IDLE):
            return
    raise AssertionError("the games did not finish")


def _drain_actor(actor, clone):
    """Every finished game through harvest_tensors(): host arrays (states, pi, z, ownership, score, root_q) and the game rows, START rebased."""
    parts, rows, base = [], [], 0
    while True:
        got = actor.harvest_tensors(clone=clone)
        assert len(got) == 4  # the 4-tuple it always was
        if len(got[3]) == 0:
            break
        aux = actor.last_harvest_aux
        assert aux._fields == ("ownership", "score", "root_q")
        assert aux.ownership.shape == (len(got[2]), actor.engine.N, actor.engine.N) and aux.score.shape == aux.root_q.shape == got[2].shape
        same = [t.data_ptr() == u.data_ptr() for t, u in zip(aux, actor.engine._harvest_aux_bufs)]
        assert not any(same) if clone else all(same)  # clone=True: private copies; else views of the engine's buffers like the rest
        games = got[3].copy()
        games[:, _abi.GR_START] += base
        base += len(got[2])
        rows.append(games)
        parts.append([t.cpu().numpy().copy() for t in got[:3] + tuple(aux)])
    assert parts
    return [np.concatenate([p[i] for p in parts]) for i in range(6)], np.concatenate(rows)


def check_actor(kind, n=5, max_steps=12):
    """SelfPlayActor(aux_targets=True): harvest_tensors() keeps its 4-tuple and leaves one aux row per sample in last_harvest_aux, the
    rows Engine.harvest(with_aux=True) of a twin actor returns and the restatement confirms; clone=True clones them; an actor without
    the feature leaves None; no drop-in engine."""
    a, b2, tw, off = (_actor(kind, n, max_steps, aux_targets=t) for t in (True, True, True, False))
    assert off.last_harvest_aux is None and a.last_harvest_aux is None and a.engine.aux_targets and not off.engine.aux_targets
    for x in (a, b2, tw, off):
        _finish(x)
    (cloned, games), (views, _) = _drain_actor(a, True), _drain_actor(b2, False)
    ref = drain(tw.engine)
    assert len(games) == G and len(cloned[2]) == len(ref["z"]) > G
    for mine, other, key in zip(cloned, views, ("states", "pi", "z", "ownership", "score", "root_q")):
        assert mine.tobytes() == other.tobytes() == ref[key].tobytes(), key
    assert games.tobytes() == ref["games"].tobytes()
    h = dict(states=cloned[0], moves=ref["moves"], ownership=cloned[3], score=cloned[4])
    for row in games:
        assert_go_game(h, row, n, max_steps)
    zs = []
    while True:
        got = off.harvest_tensors()
        if len(got[3]) == 0:
            break
        zs.append(got[2].cpu().numpy().copy())
        assert off.last_harvest_aux is None
    assert np.concatenate(zs).tobytes() == cloned[2].tobytes()
    with pytest.raises(ValueError, match="aux_targets"):
        _actor(kind, n, max_steps, aux_targets=True, engine_kw=dict(stop_after_move=True))


def _drain_games(actor):
    out = []
    while True:
        got = actor.harvest(with_moves=True)
        if not got:
            return out
        out += got


def check_actor_reference_format(kind, n=5, max_steps=12):
    """harvest(), the reference-format path, yields the same games with aux targets on as off."""
    on, off = _actor(kind, n, max_steps, aux_targets=True), _actor(kind, n, max_steps)
    _finish(on), _finish(off)
    gon, goff = _drain_games(on), _drain_games(off)
    assert len(gon) == len(goff) == G
    for (s1, st1, m1), (s2, st2, m2) in zip(gon, goff):
        assert st1 == st2 and m1 == m2 and len(s1) == len(s2) > 0
        assert all(np.array_equal(t.state, u.state) and np.array_equal(t.pi_prob, u.pi_prob) and t.value == u.value for t, u in zip(s1, s2))
