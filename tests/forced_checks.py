"""Shared drivers of the forced playouts with policy-target pruning (azsp_set_forced_playouts / azsp_read_target_policies:
EngineConfig.forced_playouts, Engine.set_forced_playouts, BatchSearch / SelfPlayActor(forced_playouts=...)).  The same functions run on the
host twin (CPU tier) and on the device (`-m gpu`).

The rule (include/azsp.h) is restated here in NumPy around the CPU oracle, from the test side: `restated()` replaces oracle.mcts._best_child
at the root by the forced selection and puts the pruning in front of oracle.mcts._finish; nothing under oracle/ is edited.  All runs use the
synthetic evaluator and injected noise and uniforms, so every comparison is bit for bit."""
import contextlib
import functools
import math

import numpy as np
import pytest
import torch

import engine_util as eu
import symmetry_checks as sc
from alpha_zero_amd import _abi
from alpha_zero_amd.core.batch_search import BatchSearch
from alpha_zero_amd.core.engine import Engine, EngineConfig
from alpha_zero_amd.core.network import AlphaZeroNet
from oracle import mcts
from synth_eval import eval_batch, make_eval_func

K = 2.0  # KataGo's factor
CB, CI = 19652.0, 1.25


# ---------------------------------------------------------------------------------------------------
# the rule, in NumPy
# ---------------------------------------------------------------------------------------------------
def floor_sqrt(x):
    """The largest integer f with f * f <= x (0 for x <= 0): a truncated square root corrected with the multiplication."""
    if not x > 0.0:
        return 0
    f = int(math.sqrt(x))
    while f > 0 and float(f) * float(f) > x:
        f -= 1
    while float(f + 1) * float(f + 1) <= x:
        f += 1
    return f


def root_scores(t, n_in_u, cb, ci):
    """oracle.mcts._scores for the root of `t`, expression for expression, with the child visit counts in the u term replaced by
    `n_in_u`; q stays W / N of the tree."""
    i = t.root
    n_self = t.get_N(i)
    pb_c = math.log((1 + n_self + cb) / cb) + ci
    u = pb_c * t.P[i] * (math.sqrt(n_self) / (1 + n_in_u))
    q = t.W[i] / np.where(t.N[i] > 0, t.N[i], 1)
    return -q + u


def forced_mask(t, legal, k):
    """(forced children of the root, children whose forcing the in-flight count v(a) ended, i.e. forced by N alone but not by N + v)."""
    r = t.root
    N = t.N[r].astype(np.float64)
    v = np.zeros(t.A)
    for mv, ch in t.child[r].items():
        v[mv] = t.vloss[ch]  # the leaves of the current batch below root move mv, duplicates counted
    t_eff = float(N.sum()) + float(t.vloss[r])
    with np.errstate(over="ignore"):  # (a very large k: the product may be inf, which forces every visited child with P > 0)
        bound = (k * t.P[r].astype(np.float64)) * np.float64(t_eff)
    n_eff = N + v
    forced = (legal == 1) & (n_eff > 0) & (n_eff * n_eff < bound)
    ended = (legal == 1) & (N > 0) & (N * N < bound) & (v > 0) & ~forced
    return forced, ended


def pruned_counts(t, legal, k, cb, ci):
    """N' of the root of `t` at the end of a search."""
    r = t.root
    N = t.N[r]
    out = N.copy()
    T = float(N.astype(np.float64).sum())
    cs = int(np.argmax(np.where(legal == 1, N, -1)))
    if legal[cs] != 1 or not N[cs] > 0:
        return out
    full = root_scores(t, N, cb, ci)
    assert full.tobytes() == mcts._scores(t, r, cb, ci).tobytes()  # the restated expression IS the selection's
    s_star = full[cs]
    for a in range(t.A):
        if legal[a] != 1 or a == cs or not N[a] > 0:
            continue
        x = (k * float(t.P[r][a])) * T
        n = int(N[a])
        # f(a) >= N(a) exactly when x >= N(a)^2 (then the scan runs down to 0); x may be inf for a very large k, which has no floor
        lo = 0 if x >= float(n) * float(n) else max(n - floor_sqrt(x), 0)
        last = n
        for m in range(n - 1, lo - 1, -1):
            rep = N.copy()
            rep[a] = m
            if root_scores(t, rep, cb, ci)[a] >= s_star:
                break
            last = m
        if last < n and last == 1:
            last = 0
        out[a] = last
    return out


@contextlib.contextmanager
def restated(k, prune=True, cb=CB, ci=CI):
    """The oracle's searches follow the rule while this is active.  Yields a dict: 'searches' = one record per finished search (N, N',
    target, in order), 'forced' = forced selections, 'ended' = selections in which v(a) ended the forcing of a child."""
    rec = dict(searches=[], forced=0, ended=0)
    best, finish = mcts._best_child, mcts._finish

    def best_child(t, i, legal, cb_, ci_, child_to_play):
        if i == t.root and k > 0:
            forced, ended = forced_mask(t, legal, k)
            rec["ended"] += int(ended.any())
            if forced.any():
                rec["forced"] += 1
                move = int(np.argmax(forced))
                if move not in t.child[i]:
                    t.child[i][move] = t._new(i, move, child_to_play)
                return t.child[i][move]
        return best(t, i, legal, cb_, ci_, child_to_play)

    def finish_search(t, env, root_legal, warm_up, deterministic, rand):
        N = t.N[t.root].copy()
        Np = pruned_counts(t, root_legal, k, cb, ci) if (k > 0 and prune) else N.copy()
        target = mcts.search_policy(Np, 1.0 if warm_up else 0.1, root_legal)
        rec["searches"].append(dict(N=N, Np=Np, target=np.asarray(target), legal=np.asarray(root_legal).copy()))
        return finish(t, env, root_legal, warm_up, deterministic, rand)

    mcts._best_child, mcts._finish = best_child, finish_search
    try:
        yield rec
    finally:
        mcts._best_child, mcts._finish = best, finish


def restated_selfplay(game, n, sims, P, G, seed, max_moves, k, root_noise, max_steps=0, num_to_win=5, prune=True, noise=None, eval_factory=None):
    """G games of the oracle's actor under the rule: (noise, uniforms, per game the per-move records, the rule's event counts).  The
    randomness is eu.oracle_selfplay's own: PCG64(seed), the Dirichlet rows (unless given), then the uniforms."""
    noise, unif, logs, results, events = eu.oracle_selfplay(game, n, sims, P, G, seed, max_moves, rule=lambda: restated(k, prune), noise=noise,
                                                            eval_factory=eval_factory, root_noise=root_noise, max_steps=max_steps, num_to_win=num_to_win)
    return noise, unif, [dict(moves=per, finished=seq is not None) for per, (seq, _) in zip(logs, results)], events


# ---------------------------------------------------------------------------------------------------
# the engine under injected randomness (eu.run_injected_search), with the target rows of every move
# ---------------------------------------------------------------------------------------------------
def target_rows(eng):
    """rows_after_move of eu.run_injected_search: the slots' target rows (SearchRun.rows[0]), nothing while forced playouts were never on."""
    return (eng.target_policies().cpu().numpy(),) if eng.forced_playouts else None


def same_run(a, b, targets=True):
    """Bit for bit: two SearchRuns' logs, harvest, evaluations per ply, counters (and the rows read after every move)."""
    try:
        sc.assert_same_outputs(a, b)
    except AssertionError:
        return False
    as_bytes = lambda run: [[[r.tobytes() for r in per] for per in arr] for arr in run.rows]  # noqa: E731
    return not targets or as_bytes(a) == as_bytes(b)


# ---------------------------------------------------------------------------------------------------
# 1. + 4. the engine against the restated search; the pruning invariants on every search
# ---------------------------------------------------------------------------------------------------
# the smallest shapes that reach every code path: one element per lane (A = 26), the second lane element and the float64 policy
# (A = 82), the float32 policy path (Gomoku), six bitboard words (19x19).  Go games end at max_steps, so every game is harvested.
SHAPES = {
    "go5": dict(game="go", n=5, sims=32, G=2, max_moves=12, max_steps=12, seed=31),
    "go9": dict(game="go", n=9, sims=48, G=1, max_moves=5, max_steps=5, seed=35),
    "gomoku7": dict(game="gomoku", n=7, sims=24, G=1, max_moves=14, num_to_win=3, seed=33),
    "go19": dict(game="go", n=19, sims=64, G=1, max_moves=3, max_steps=3, seed=40),
    "go5_short": dict(game="go", n=5, sims=16, G=1, max_moves=3, max_steps=3, seed=43),  # check_large_factor
}
CASES = [("go5", 1), ("go5", 4), ("go9", 1), ("go9", 4), ("go9", 8), ("gomoku7", 1), ("gomoku7", 4), ("go19", 4)]


_selfplay_args, _shape_kw = eu.shape_table(SHAPES)


@functools.lru_cache(maxsize=None)
def _restated_case(shape, P, root_noise, k=K, prune=True):
    args, kw = _selfplay_args(shape, P)
    return restated_selfplay(*args, k, root_noise, prune=prune, **kw)


def _engine_kw(shape, P, root_noise):
    return _shape_kw(shape, P, root_noise=root_noise)


def assert_pruning_invariants(move, A, f32):
    """N' <= N, N'(c*) = N(c*), no reduced child left at 1, the target sums to 1."""
    N, Np, legal = move["child_N"], move["Np"], move["legal"]
    assert np.all(Np <= N) and np.all(Np >= 0)
    cs = int(np.argmax(np.where(legal == 1, N, -1)))
    assert Np[cs] == N[cs]
    assert not np.any((Np < N) & (Np == 1))
    eps = np.finfo(np.float32 if f32 else np.float64).eps
    assert abs(float(np.asarray(move["target"], dtype=np.float64).sum()) - 1.0) <= A * eps


def check_restatement(kind, shape, P, root_noise, k=K, expect_ended=True, read_targets=True):
    """The engine with forced_playouts = k (2) against the restated search over consecutive moves with tree reuse: child_N, the unpruned
    pi, root and child Q, the moves; target_pi exactly; the harvested pi rows against the float32 cast of the target.
    read_targets=False is for searches in which a kept sub-tree can hold a whole budget, so that a slot makes two moves in one round and
    the driver cannot read its target row in between: the targets are then compared through the harvested rows only."""
    s = SHAPES[shape]
    noise, unif, want, events = _restated_case(shape, P, root_noise, k)
    got = eu.run_injected_search(kind, noise, unif, eval_batch, forced_playouts=k, rows_after_move=target_rows if read_targets else None,
                                 **_engine_kw(shape, P, root_noise))
    A = noise.shape[2]
    f32 = s["game"] != "go"
    assert events["forced"] > 0
    if P > 1 and expect_ended:
        assert events["ended"] > 0, "no select phase in which the in-flight count ended the forcing of a child"
    by_slot = {int(r[_abi.GR_SLOT]): r for r in got.harvest[3]}
    for g, game in enumerate(want):
        e_moves = got.logs[g]
        t_rows = got.rows[0][g] if read_targets else [np.asarray(m["target"], dtype=np.float64) for m in game["moves"]]
        assert len(e_moves) == len(game["moves"]) == len(t_rows) >= 2, (g, len(e_moves), len(game["moves"]), len(t_rows))
        for k, (e, o, tp) in enumerate(zip(e_moves, game["moves"], t_rows)):
            where = (shape, P, root_noise, g, k)
            assert e["move"] == o["move"], where
            assert np.array_equal(e["child_N"], o["child_N"]), where
            assert e["root_q"] == o["root_q"] and e["child_q"] == o["child_q"], where
            assert e["pi"].tobytes() == np.asarray(o["pi"], dtype=np.float64).tobytes(), where
            assert tp.dtype == np.float64 and tp.tobytes() == np.asarray(o["target"], dtype=np.float64).tobytes(), where
            assert_pruning_invariants(o, A, f32)
            assert abs(tp.sum() - 1.0) <= A * np.finfo(np.float32 if f32 else np.float64).eps, where
        if game["finished"]:
            rows = eu.samples_of(by_slot[g], got.harvest[1])
            assert rows.tobytes() == np.stack([np.asarray(m["target"], dtype=np.float32) for m in game["moves"]]).tobytes(), (shape, P, g)
        else:
            assert g not in by_slot
    if s["game"] == "go":
        assert all(game["finished"] for game in want)


def check_pruning_is_not_vacuous():
    """A check of the reference set, not of the engine (it runs the NumPy restatement and the oracle only, so it passes with or without
    the feature): what check_restatement compares the engine with is worth comparing with.  Covers go5 P = 1 / 4 and gomoku7 P = 1 with
    root noise.  Over the searches of these restated cases: at least one has N' != N, at least one has a child pruned to 0, and the forced search
    is another search than the plain one."""
    changed = zeroed = 0
    for shape, P in (("go5", 1), ("go5", 4), ("gomoku7", 1)):
        for game in _restated_case(shape, P, True)[2]:
            for m in game["moves"]:
                changed += int(np.any(m["Np"] != m["child_N"]))
                zeroed += int(np.any((m["Np"] == 0) & (m["child_N"] > 0)))
    assert changed > 0 and zeroed > 0, (changed, zeroed)
    plain = _restated_case("go5", 4, True, 0.0)[2]
    forced = _restated_case("go5", 4, True)[2]
    assert any(not np.array_equal(a["child_N"], b["child_N"]) for ga, gb in zip(plain, forced) for a, b in zip(ga["moves"], gb["moves"]))
    assert floor_sqrt(24.999999) == 4 and floor_sqrt(25.0) == 5 and floor_sqrt(0.0) == 0 and floor_sqrt(-1.0) == 0 and floor_sqrt(0.99) == 0


LARGE_FACTORS = [1e40, 1e300, 1.7976931348623157e308]


def check_large_factor(kind, k, P, root_noise):
    """Every finite k is accepted, so a search with a very large one must finish, and as the restated search: (k P(a)) T is then far
    beyond any N(a)^2 -- 8.5e37 is where a 64-bit truncation of its square root ends, and with the largest double it is inf -- so every
    visited child with P > 0 is forced in every selection (the in-flight count never ends a forcing) and every such child but c* may be
    pruned down to 0, for as long as its score stays below S*.  Only min(f(a), N(a)) enters the pruning: its cost stays N(a) scores."""
    assert np.isfinite(k) and k >= 1e40
    # P = 4: the one forced child holds 21 visits against a budget of 20, so the next move follows in the same round (see read_targets)
    check_restatement(kind, "go5_short", P, root_noise, k=k, expect_ended=False, read_targets=P == 1)
    assert SHAPES["go5_short"]["max_steps"] == SHAPES["go5_short"]["max_moves"]  # every game ends and is harvested: the rows are compared
    # the factor was in effect: on the fresh root of move 0 the first child visited is forced in every later selection, so it holds
    # every visit of the search (with k = 2 the same search spreads over five children or more)
    for game in _restated_case("go5_short", P, root_noise, k)[2]:
        assert np.count_nonzero(game["moves"][0]["child_N"]) == 1


# ---------------------------------------------------------------------------------------------------
# 2. off is the parent
# ---------------------------------------------------------------------------------------------------
def check_off_is_the_parent(kind, shape="go5", P=4):
    """k = 0, and k = 2 used and then turned off, give the logs, harvests and counters of an engine that never heard of the feature;
    prune_target = 0 gives a harvested pi equal to the logged pi of the (forced) search."""
    noise, unif, _, _ = _restated_case(shape, P, True)
    kw = _engine_kw(shape, P, True)
    never = eu.run_injected_search(kind, noise, unif, eval_batch, rows_after_move=target_rows, **kw)
    assert never.rows == () and sum(len(g) for g in never.logs) >= 4

    def used_then_off(eng):
        eng.set_forced_playouts(K)
        eng.reset_games()
        eng.priors.fill_(1.0 / eng.A)
        eng.select()
        for _ in range(12):
            eng.round()
        eng.set_forced_playouts(0.0)

    zero = eu.run_injected_search(kind, noise, unif, eval_batch, setup=lambda eng: eng.set_forced_playouts(0.0), rows_after_move=target_rows, **kw)
    off = eu.run_injected_search(kind, noise, unif, eval_batch, setup=used_then_off, **kw)
    cfg0 = eu.run_injected_search(kind, noise, unif, eval_batch, forced_playouts=0.0, rows_after_move=target_rows, **kw)
    for other in (zero, off, cfg0):
        assert same_run(never, other, targets=False)
    on = eu.run_injected_search(kind, noise, unif, eval_batch, forced_playouts=K, rows_after_move=target_rows, **kw)
    assert not same_run(never, on, targets=False)
    unpruned = eu.run_injected_search(kind, noise, unif, eval_batch, setup=lambda eng: eng.set_forced_playouts(K, prune_target=False),
                                      rows_after_move=target_rows, **kw)
    assert unpruned.counters == on.counters  # the same searches: pruning touches the target only
    n_rows = 0
    for row in unpruned.harvest[3]:
        g = int(row[_abi.GR_SLOT])
        rows = eu.samples_of(row, unpruned.harvest[1])
        assert rows.tobytes() == np.stack([m["pi"].astype(np.float32) for m in unpruned.logs[g]]).tobytes()
        assert all(t.tobytes() == m["pi"].tobytes() for t, m in zip(unpruned.rows[0][g], unpruned.logs[g]))
        assert all(a["pi"].tobytes() == b["pi"].tobytes() and a["move"] == b["move"] for a, b in zip(unpruned.logs[g], on.logs[g]))
        n_rows += len(rows)
    assert n_rows >= 4 and unpruned.harvest[1].tobytes() != on.harvest[1].tobytes()


# ---------------------------------------------------------------------------------------------------
# 3. a case that discriminates
# ---------------------------------------------------------------------------------------------------
def corner_eval(x, A):
    """Uniform priors; a position with a stone on point 0 is lost for the stone's owner: value +0.9 for the player to move when the
    stone is the opponent's (plane 1), -0.9 when it is the mover's own (plane 0), 0 without one."""
    x = np.asarray(x)
    v = np.where(x[:, 1, 0, 0] == 1, 0.9, np.where(x[:, 0, 0, 0] == 1, -0.9, 0.0)).astype(np.float32)
    return np.full((len(x), A), np.float32(1.0 / A), dtype=np.float32), v


def corner_eval_func(A):
    def f(obs, batched=False):
        p, v = corner_eval(np.asarray(obs) if batched else np.asarray(obs)[None], A)
        return (list(p), [float(t) for t in v]) if batched else (p[0], float(v[0]))

    return f


def check_discriminating_case(kind, sims=48):
    """Go 5x5, P = 1, the noise row one-hot on action 0 (P(0) = 0.75 / 26 + 0.25), and an evaluator under which the move to point 0
    loses: the plain search leaves action 0 with the one or two visits its prior buys, far below sqrt(k P(0) T).  With k = 2 the
    engine ends with N(0)^2 >= k P(0) (T - 1); the plain engine on the same inputs violates the bound, and both are the restated
    searches."""
    A = 26
    noise = np.zeros((1, 2, A))
    noise[:, :, 0] = 1.0
    unif = np.random.Generator(np.random.PCG64(7)).random((1, 2, 16))
    kw = dict(game="go", board_size=5, num_parallel=1, num_simulations=sims, max_plies=1, warm_up_steps=4, force_resign_disabled=1)
    p0 = float(np.float64(np.float32(1.0 / A) * np.float32(0.75)) + 1.0 * 0.25)  # the noisy root prior of action 0, as the search forms it
    n_end = {}
    for k in (K, 0.0):
        got = eu.run_injected_search(kind, noise, unif, corner_eval, rows_after_move=target_rows, **(dict(kw, forced_playouts=k) if k else kw))
        cn = got.logs[0][0]["child_N"]
        want = restated_selfplay("go", 5, sims, 1, 1, 7, 1, k, True, noise=noise, eval_factory=corner_eval_func)[2][0]["moves"][0]
        assert np.array_equal(cn, want["child_N"]) and got.logs[0][0]["pi"].tobytes() == np.asarray(want["pi"], np.float64).tobytes()
        n_end[k] = (float(cn[0]), float(cn.sum()))
    n0, T = n_end[K]
    assert n0 * n0 >= K * p0 * (T - 1), (n0, T, p0)
    n0, T = n_end[0.0]
    assert n0 >= 1 and n0 * n0 < K * p0 * (T - 1), (n0, T, p0)  # the plain search violates the bound: the case needs the feature


# ---------------------------------------------------------------------------------------------------
# 5. playout cap
# ---------------------------------------------------------------------------------------------------
def check_playout_cap(kind, P=1, G=12):
    """Forced playouts on: a cap with full_prob = 0 equals the same cap with them off (fast moves are neither forced nor pruned), one
    with full_prob = 1 equals the forced search without a cap, and in between the fast samples' pi rows are the plain policy and the
    full ones the pruned target -- the rows of an actor that forces without pruning, except on full moves.

    What pins the values of a pruned row: full_prob = 1 against the uncapped forced actor here, and check_restatement, which compares
    target_pi and the harvested rows with the restated pruning bit for bit.  The in-between run pins the fast rows exactly (the plain
    policy) and the classes; of its full rows it checks only that pruning added no support and changed at least one of them.  Restating
    their pruning from the move log would need the root's W row, which the log does not carry."""
    import budget_checks as bk

    def played(**kw):
        a = bk._actor(kind, P, G=G, **kw)
        cnt = bk._play_out(a)
        logs = [[a.engine.get_search(g, k)[0] for k in range(bk.MAX_STEPS)] for g in range(G)]
        out = bk._drain_engine(a)
        a.engine.close()
        return out, cnt, logs

    fast_on, c1, _ = played(playout_cap=(bk.FAST, 0.0), forced_playouts=K)
    fast_off, c2, _ = played(playout_cap=(bk.FAST, 0.0))
    assert bk._same_tensors(fast_on, fast_off) and c1 == c2 and (fast_on[5] == 0).all()
    full_on, c3, _ = played(playout_cap=(bk.FAST, 1.0), forced_playouts=K)
    forced, c4, _ = played(forced_playouts=K)
    plain, c5, _ = played()
    assert bk._same_tensors(full_on, forced) and c3 == c4 and (full_on[5] == 1).all()
    assert not bk._same_tensors(forced[:3], plain[:3]) and c4 != c5
    mixed, c6, logs = played(playout_cap=(bk.FAST, 0.5), forced_playouts=K)
    unpruned, c7, _ = played(playout_cap=(bk.FAST, 0.5), forced_playouts=K, prune_policy_target=False)
    assert c6 == c7 and all(bk._same_tensors([mixed[i]], [unpruned[i]]) for i in (0, 2, 3, 4, 5))  # the same games, moves and classes
    pi, games, klass = mixed[1], mixed[3], mixed[5]
    assert (klass == 1).any() and (klass == 0).any()
    changed = 0
    for row in games:
        g, s0 = int(row[_abi.GR_SLOT]), int(row[_abi.GR_START])
        for ply in range(int(row[_abi.GR_LENGTH])):
            logged = logs[g][ply].astype(np.float32)
            assert unpruned[1][s0 + ply].tobytes() == logged.tobytes(), (g, ply)
            if klass[s0 + ply] == 0:
                assert pi[s0 + ply].tobytes() == logged.tobytes(), (g, ply)  # a fast move: the plain policy
            else:
                assert not np.any((pi[s0 + ply] > 0) & (logged == 0)), (g, ply)  # pruning only takes visits away
                changed += int(pi[s0 + ply].tobytes() != logged.tobytes())
    assert changed > 0


# ---------------------------------------------------------------------------------------------------
# 6. leaf symmetry
# ---------------------------------------------------------------------------------------------------
def check_leaf_symmetry(kind, op=3, shape="go5", P=4):
    """The forced search under a fixed op equals the forced search around the wrapped evaluator."""
    noise, unif, _, _ = _restated_case(shape, P, True)
    kw = dict(_engine_kw(shape, P, True), forced_playouts=K, rows_after_move=target_rows)
    under_op = eu.run_injected_search(kind, noise, unif, eval_batch, leaf_symmetry=op, **kw)
    wrapped = eu.run_injected_search(kind, noise, unif, sc.wrapped_eval(op, SHAPES[shape]["n"]), **kw)
    plain = eu.run_injected_search(kind, noise, unif, eval_batch, **kw)
    assert same_run(under_op, wrapped) and not same_run(under_op, plain)


# ---------------------------------------------------------------------------------------------------
# 7. BatchSearch and drop-in
# ---------------------------------------------------------------------------------------------------
def check_batch_search(kind, game="go", n=5, P=1, budgets=(24, 9, 16, 24)):
    """BatchSearch(forced_playouts = 2) on the empty board in every slot, slots with different budgets, noise rows and warm flags, two
    moves with tree reuse: pi, child_N, root Q and target_pi of every slot are those of the restated oracle search; target_pi is None
    when off."""
    A = eu.num_actions(game, n)
    G = len(budgets)
    b, dev = eu.backend(kind)
    rng = np.random.Generator(np.random.PCG64(41))
    noise = rng.dirichlet(np.full(A, 0.03), size=(2, G))
    warm = np.array([s % 2 == 0 for s in range(G)])
    boards, hist, pos = eu.empty_positions(n, G)
    ef = make_eval_func(A)
    off = BatchSearch(game, n, G, max(budgets), num_parallel=P, root_noise=True, binding=b, device=dev)
    assert np.all(off.load(boards, hist, pos) == _abi.SS_OK)
    off.search(ef, noise=noise[0], warm_up=warm, num_simulations=list(budgets))
    assert off.results().target_pi is None
    off_cn = off.results().cpu()[1]
    off.close()
    bs = BatchSearch(game, n, G, max(budgets), num_parallel=P, root_noise=True, binding=b, device=dev, forced_playouts=K)
    assert np.all(bs.load(boards, hist, pos) == _abi.SS_OK)
    assert not bs.eng.target_policies().cpu().numpy().any()  # zero before the first finished search
    envs, trees = [eu.make_oracle_env(game, n) for _ in range(G)], [None] * G
    differs = 0
    for move in range(2):
        bs.search(ef, noise=noise[move], warm_up=warm, num_simulations=list(budgets))
        res = bs.results()
        pi, cn, rq = res.cpu()
        tp = res.target_pi.cpu().numpy()
        assert tp.dtype == np.float64 and tp.shape == (G, A) and list(bs.slots) == list(range(G))
        moves = []
        for s in range(G):
            with restated(K) as rec:
                kw = dict(env=envs[s], eval_func=ef, root_node=trees[s], c_puct_base=CB, c_puct_init=CI, num_simulations=budgets[s],
                          root_noise=True, warm_up=bool(warm[s]), deterministic=True, rand=mcts.InjectedRand(noise[move, s], []))
                mv, opi, orq, _, trees[s] = mcts.parallel_uct_search(num_parallel=P, **kw) if P > 1 else mcts.uct_search(**kw)
            srec = rec["searches"][0]
            where = (game, P, move, s)
            assert np.array_equal(cn[s], srec["N"]) and rq[s] == float(orq), where
            assert pi[s].tobytes() == np.asarray(opi).astype(pi.dtype).tobytes(), where
            assert tp[s].tobytes() == np.asarray(srec["target"], dtype=np.float64).tobytes(), where
            differs += int(tp[s].tobytes() != np.asarray(pi[s], dtype=np.float64).tobytes())
            assert mv == int(np.argmax(cn[s]))
            moves.append(mv)
            envs[s].step(mv)
        if move == 0:
            assert not np.array_equal(cn, off_cn)
        _, reusable = bs.commit(moves)
        assert reusable.all() and all(t is not None for t in trees)
    assert differs > 0
    bs.close()


def check_resident_equals_callback(kind):
    """The resident loop (an evaluator with device_eval) and the host callback loop run the same forced searches: pi, child_N, Q, target_pi."""
    import batch_search_checks as bc
    from arena_checks import SynthDeviceEvaluator

    b, dev = eu.backend(kind)
    boards, hist, pos = bc.positions("go", 5, 8, 6)
    rows = {}
    for route, ev in (("resident", SynthDeviceEvaluator(26, 2.0)), ("callback", make_eval_func(26))):
        bs = BatchSearch("go", 5, 6, 32, num_parallel=4, binding=b, device=dev, forced_playouts=K)
        assert np.all(bs.load(boards, hist, pos) == _abi.SS_OK)
        bs.search(ev, num_simulations=[32, 12, 20, 32, 12, 20])
        res = bs.results()
        rows[route] = tuple(x.tobytes() for x in res.cpu()) + (res.target_pi.cpu().numpy().tobytes(),)
        bs.close()
    assert rows["resident"] == rows["callback"]


def check_resident_identity_gpu():
    """BatchSearch(forced_playouts = 2) behind a DeviceEvaluator on a small 9x9 fp32-class network: the resident loop equals the host
    callback loop around the same evaluator, target_pi included, and is another search than the plain one.  (Device only.)"""
    import batch_search_checks as bc

    inf, ev = eu.small_go9_device_evaluator()
    boards, hist, pos = bc.positions("go", 9, 8, 6)
    rows = {}
    for route, forced in (("resident", K), ("callback", K), ("plain", None)):
        bs = BatchSearch("go", 9, 6, 48, num_parallel=4, forced_playouts=forced)
        assert np.all(bs.load(boards, hist, pos) == _abi.SS_OK)
        bs.search((lambda s, batched=False: ev(s, batched)) if route == "callback" else ev)
        res = bs.results()
        rows[route] = tuple(x.tobytes() for x in res.cpu()) + ((res.target_pi.cpu().numpy().tobytes(),) if forced else ())
        bs.close()
    assert rows["resident"] == rows["callback"]
    assert rows["resident"][:3] != rows["plain"]
    assert inf.split_range_status(reset=True)[0] == 0


# ---------------------------------------------------------------------------------------------------
# 8. production randomness: the device and the host twin
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def seeded_actor_games(kind, P=4, G=8):
    """A seeded actor without injection (Go 5x5, forced playouts and a playout cap on) plays one game per slot: the drained harvest."""
    import budget_checks as bk

    a = bk._actor(kind, P, G=G, seed=9, rank=1, playout_cap=(bk.FAST, 0.5), forced_playouts=K)
    cnt = bk._play_out(a)
    out = bk._drain_engine(a)
    a.engine.close()
    return out, cnt


def check_seeded_actor(kind):
    """The seeded run is reproducible on its backend, every pi row sums to 1 and both classes occur; on the device it equals the host twin's."""
    import budget_checks as bk

    out, cnt = seeded_actor_games(kind)
    assert len(out[3]) == 8 and np.allclose(out[1].sum(1), 1.0, atol=1e-6) and (out[5] == 1).any() and (out[5] == 0).any()
    host, host_cnt = seeded_actor_games("host")
    if kind != "host":
        assert bk._same_tensors(out, host) and cnt == host_cnt
    else:
        seeded_actor_games.cache_clear()
        again, again_cnt = seeded_actor_games("host")
        assert bk._same_tensors(out, again) and cnt == again_cnt


# ---------------------------------------------------------------------------------------------------
# 9. refusals
# ---------------------------------------------------------------------------------------------------
def check_refusals(kind):
    """Negative, NaN and infinite k are AZSP_EINVAL at the ABI and ValueError in Python, before anything is built."""
    import ctypes as C

    import budget_checks as bk

    b, dev = eu.backend(kind)
    eng = Engine(b, EngineConfig(game="go", board_size=5, num_games=2, num_parallel=2, num_simulations=8), device=dev)
    fp = lambda k, prune=1: b.dll.azsp_set_forced_playouts(eng.h, C.c_double(k), prune)  # noqa: E731
    out = torch.zeros((2, 26), dtype=torch.float64, device=dev)
    assert b.dll.azsp_read_target_policies(eng.h, out.data_ptr(), None) == -1  # never enabled: no rows
    assert fp(0.0) == 0 and b.dll.azsp_read_target_policies(eng.h, out.data_ptr(), None) == -1
    assert [fp(-1.0), fp(-1e-300), fp(float("nan")), fp(float("inf")), fp(float("-inf"))] == [-1] * 5
    assert b.dll.azsp_set_forced_playouts(None, C.c_double(2.0), 1) == -1
    assert [fp(2.0), fp(0.5, 0), fp(1e6), fp(0.0)] == [0] * 4
    assert b.dll.azsp_read_target_policies(eng.h, out.data_ptr(), None) == 0 and not out.cpu().numpy().any()
    assert b.dll.azsp_read_target_policies(eng.h, None, None) == -1
    for bad in (-1, -0.5, float("nan"), float("inf"), "2", True, [2.0]):
        with pytest.raises(ValueError, match=r"forced_playouts must be None \(off\) or a finite number k >= 0"):
            eng.set_forced_playouts(bad)
        with pytest.raises(ValueError, match="forced_playouts"):
            Engine(b, EngineConfig(game="go", board_size=5, num_games=1, num_parallel=1, num_simulations=4, forced_playouts=bad), device=dev)
        with pytest.raises(ValueError, match="forced_playouts"):
            BatchSearch("go", 5, 2, 8, binding=b, device=dev, forced_playouts=bad)
    net = AlphaZeroNet((17, 5, 5), 26, 1, 8, 8)
    for bad in (-2.0, float("nan")):
        with pytest.raises(ValueError, match="forced_playouts"):
            bk._actor(kind, 1, net=net, G=2, forced_playouts=bad)
    eng.set_forced_playouts(np.float32(1.5))
    eng.set_forced_playouts(2)
    eng.set_forced_playouts(None)
    eng.close()
