"""Shared drivers of the leaf symmetry (azsp_set_leaf_symmetry / azsp_leaf_symmetries: EngineConfig.leaf_symmetry, Engine.set_leaf_symmetry,
BatchSearch / SelfPlayActor(leaf_symmetry=...)).  The same functions run on the host twin (CPU tier) and on the device (`-m gpu`).

The rule under test: a search with symmetry k around an evaluator E equals, bit for bit, the plain search around the evaluator
"transform the planes by k, run E, map the priors back by inv(k)".  The transforms are restated here with NumPy's flip / rot90 /
swapaxes, not taken from the engine; E is the synthetic evaluator that pins the goldens (synth_eval.eval_batch).  Every comparison is exact."""
import functools
import warnings

import numpy as np
import pytest
import torch

import batch_search_checks as bc
import engine_util as eu
from alpha_zero_amd import _abi
from alpha_zero_amd.core.batch_search import BatchSearch
from alpha_zero_amd.core.engine import Engine, EngineConfig
from alpha_zero_amd.core.network import AlphaZeroNet
from budget_checks import SynthActor, philox4x32_10
from synth_eval import eval_batch, make_eval_func

INV = (0, 1, 2, 5, 4, 3, 6, 7)  # inv(op): the two quarter turns swap


# ---------------------------------------------------------------------------------------------------
# the eight transforms, in NumPy
# ---------------------------------------------------------------------------------------------------
def d_planes(x, op):
    """D_op on the last two axes: out[..., i, j] = in[..., src_op(i, j)] (include/azsp.h azsp_dihedral)."""
    if op == 1:
        y = np.flip(x, -1)  # in[i][n-1-j]
    elif op == 2:
        y = np.flip(x, -2)  # in[n-1-i][j]
    elif op in (3, 4, 5):
        y = np.rot90(x, op - 2, axes=(-2, -1))  # counter-clockwise quarter turns: in[j][n-1-i], in[n-1-i][n-1-j], in[n-1-j][i]
    elif op == 6:
        y = np.swapaxes(x, -1, -2)  # in[j][i]
    elif op == 7:
        y = np.flip(np.flip(np.swapaxes(x, -1, -2), -1), -2)  # in[n-1-j][n-1-i]
    else:
        assert op == 0
        y = x
    return np.ascontiguousarray(y)


def d_policy(p, op, n):
    """D_op on policy rows [..., A]: the n * n board entries move like a plane, a pass column stays."""
    out = np.array(p, copy=True)
    out[..., : n * n] = d_planes(p[..., : n * n].reshape(p.shape[:-1] + (n, n)), op).reshape(p.shape[:-1] + (n * n,))
    return out


def check_transforms_are_the_documented_maps():
    """The NumPy restatement against the index formulas of include/azsp.h, and inv(op) against composition: a mistake in this file's
    own yardstick would otherwise cancel out in every comparison below."""
    n = 5
    x = np.arange(n * n).reshape(n, n)
    src = {0: lambda i, j: (i, j), 1: lambda i, j: (i, n - 1 - j), 2: lambda i, j: (n - 1 - i, j), 3: lambda i, j: (j, n - 1 - i),
           4: lambda i, j: (n - 1 - i, n - 1 - j), 5: lambda i, j: (n - 1 - j, i), 6: lambda i, j: (j, i), 7: lambda i, j: (n - 1 - j, n - 1 - i)}
    for op in range(8):
        want = np.array([[x[src[op](i, j)] for j in range(n)] for i in range(n)])
        assert np.array_equal(d_planes(x, op), want), op
        assert np.array_equal(d_planes(d_planes(x, op), INV[op]), x), op
    p = np.arange(26, dtype=np.float32)[None]
    assert d_policy(p, 3, n)[0, 25] == 25 and np.array_equal(d_policy(p, 3, n)[0, :25], d_planes(x, 3).reshape(-1))


def wrapped_eval(op, n):
    """x -> (D_inv(op)(p), v) with (p, v) = E(D_op(x)): what a search under the fixed op `op` makes of E."""
    def f(x, A):
        p, v = eval_batch(d_planes(x, op), A)
        return d_policy(p, INV[op], n), v

    return f


# ---------------------------------------------------------------------------------------------------
# 1. fixed op == plain search around the wrapped evaluator
# ---------------------------------------------------------------------------------------------------
SHAPES = {
    # whole games (Go 5x5 ends at 50 steps); P = 4
    "go5": dict(kw=dict(game="go", board_size=5, num_parallel=4, num_simulations=32, warm_up_steps=4), G=2, M=51, seed=21),
    # 16 rows = 5 tiles of three boards and a single: every sub-tile position and a partly filled last tile
    "go9": dict(kw=dict(game="go", board_size=9, num_parallel=8, num_simulations=64, warm_up_steps=4, max_plies=6), G=2, M=7, seed=22),
    # no pass column; P = 1 (uct_search semantics)
    "gomoku7": dict(kw=dict(game="gomoku", board_size=7, num_parallel=1, num_simulations=40, warm_up_steps=4, max_plies=10), G=2, M=11, seed=23),
    # six plane words, several lane passes per plane
    "go19": dict(kw=dict(game="go", board_size=19, num_parallel=2, num_simulations=8, warm_up_steps=4, max_plies=2), G=2, M=3, seed=24),
}
SHAPE_DTYPES = {"go5": (_abi.FEAT_I8,), "go9": (_abi.FEAT_I8, _abi.FEAT_BF16_TILED, _abi.FEAT_F16_SPLIT), "gomoku7": (_abi.FEAT_I8,),
                "go19": (_abi.FEAT_I8,)}
OTHER_DTYPES = (_abi.FEAT_F32, _abi.FEAT_BF16, _abi.FEAT_F16, _abi.FEAT_F16_TILED)


def _randomness(shape):
    s = SHAPES[shape]
    A = eu.num_actions(s["kw"]["game"], s["kw"]["board_size"])
    rng = np.random.Generator(np.random.PCG64(s["seed"]))
    return rng.dirichlet(np.full(A, 0.03), size=(s["G"], s["M"])), rng.random((s["G"], s["M"], 16))


def _run(kind, shape, evaluator, on_features=None, **kw):
    """run_injected_search on `shape`, keeping the decoded features of every round: (outputs, [features per round])."""
    noise, unif = _randomness(shape)
    feats = []

    def see(rnd, f, eng):
        feats.append(f.copy())
        if on_features is not None:
            on_features(rnd, f, eng)

    out = eu.run_injected_search(kind, noise, unif, evaluator, on_features=see, **SHAPES[shape]["kw"], **kw)
    return out, feats


@functools.lru_cache(maxsize=None)
def _plain_run(kind, shape, op):
    """The yardstick, once per (backend, shape, op): the mode off, int8 planes, evaluator wrapped by `op` (op None: E itself)."""
    n = SHAPES[shape]["kw"]["board_size"]
    return _run(kind, shape, eval_batch if op is None else wrapped_eval(op, n), feature_dtype=_abi.FEAT_I8)


def assert_same_outputs(a, b, where=None):
    """Bit for bit, two SearchRuns: logs (pi, child_N, root_q, child_q, move), harvest (states, pi, z, game rows), evaluations per ply,
    counters."""
    (la, ha, na, ca), (lb, hb, nb, cb) = a[:4], b[:4]
    assert len(la) == len(lb)
    for gi, (ga, gb) in enumerate(zip(la, lb)):
        assert len(ga) == len(gb) > 0, (where, gi, len(ga), len(gb))
        for k, (x, y) in enumerate(zip(ga, gb)):
            assert x["move"] == y["move"], (where, gi, k, x["move"], y["move"])
            assert x["pi"].tobytes() == y["pi"].tobytes() and x["child_N"].tobytes() == y["child_N"].tobytes(), (where, gi, k)
            assert np.float64(x["root_q"]).tobytes() == np.float64(y["root_q"]).tobytes(), (where, gi, k)
            assert np.float64(x["child_q"]).tobytes() == np.float64(y["child_q"]).tobytes(), (where, gi, k)
    for x, y in zip(ha, hb):
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), where
    assert np.array_equal(na, nb) and ca == cb, (where, ca, cb)


def check_fixed_op(kind, shape, op, dtypes=None):
    """leaf_symmetry = op around E against the mode off around the wrapped evaluator, for every feature layout of the shape; the
    decoded features of every round are D_op of the plain run's."""
    plain, plain_feats = _plain_run(kind, shape, op)
    assert sum(len(g) for g in plain.logs) >= 2 and plain.counters["leaves"] > 0
    for dt in dtypes or SHAPE_DTYPES[shape]:
        got, feats = _run(kind, shape, eval_batch, feature_dtype=dt, leaf_symmetry=op)
        assert_same_outputs(got, plain, (shape, op, dt))
        assert len(feats) == len(plain_feats)
        for rnd, (f, g) in enumerate(zip(feats, plain_feats)):
            assert np.array_equal(f, d_planes(g, op)), (shape, op, dt, rnd)
    if op != 0:  # the comparison can fail: the plain run around E itself is another search
        base = _plain_run(kind, shape, None)[0]
        assert any(x["child_N"].tobytes() != y["child_N"].tobytes() for ga, gb in zip(plain.logs, base.logs) for x, y in zip(ga, gb))


# ---------------------------------------------------------------------------------------------------
# 2. random mode == plain search, when the evaluator undoes every row's op
# ---------------------------------------------------------------------------------------------------
def check_random_mode(kind, shape, dtype=_abi.FEAT_I8, switch=(12, 20, 28)):
    """leaf_symmetry = "random": the evaluator wrapper reads Engine.leaf_symmetries() every round, undoes each row's op, calls E and
    transforms the priors forward -- the engine maps them back -- so the whole run equals the plain run around E.  At the rounds
    `switch` the mode goes "random" -> 3 -> off -> "random"; the rows selected before a switch are in flight across it and keep the op
    they were written with."""
    n = SHAPES[shape]["kw"]["board_size"]
    state, seen = {}, {"random": [], 3: [], None: []}
    plan = {switch[0]: 3, switch[1]: None, switch[2]: "random"}
    mode = ["random"]

    def on_features(rnd, feats, eng):
        ops = eng.leaf_symmetries().cpu().numpy()
        valid = eng.valid.cpu().numpy().astype(bool)
        assert ops.dtype == np.uint8 and ops.shape == (eng.rows,) and ops.max() <= 7 and not ops[~valid].any()
        state["ops"] = ops[valid]
        seen[mode[0]].append(ops[valid].copy())
        if rnd in plan:  # holds for the rows of the NEXT select; this round's rows are expanded under the ops read above
            mode[0] = plan[rnd]
            eng.set_leaf_symmetry(mode[0])

    def evaluator(x, A):
        ops = state["ops"]
        assert len(ops) == len(x)
        true = np.stack([d_planes(x[r], INV[ops[r]]) for r in range(len(x))])
        p, v = eval_batch(true, A)
        return np.stack([d_policy(p[r], ops[r], n) for r in range(len(x))]), v

    got, feats = _run(kind, shape, evaluator, on_features=on_features, feature_dtype=dtype, leaf_symmetry="random")
    plain, plain_feats = _plain_run(kind, shape, None)
    assert_same_outputs(got, plain, (shape, dtype))
    assert len(feats) == len(plain_feats) > switch[2] + 4
    rnd_ops = np.concatenate(seen["random"])
    assert len(np.unique(rnd_ops)) >= 4 and len(rnd_ops) > 20  # the wrapper had something to undo
    assert all((o == 3).all() for o in seen[3]) and sum(len(o) for o in seen[3]) > 0
    assert all((o == 0).all() for o in seen[None]) and sum(len(o) for o in seen[None]) > 0
    assert any(not np.array_equal(f, g) for f, g in zip(feats, plain_feats))


# ---------------------------------------------------------------------------------------------------
# 3. the stream
# ---------------------------------------------------------------------------------------------------
STREAM_G, STREAM_P = 40, 8  # 40 games cross a 32-game launch boundary


def _uniform_rounds(kind, rounds, seed, rank, mode="random", probe=False):
    """A production-randomness engine (no injection) driven with uniform priors and zero values: per round the (rows, ops) it wrote.
    probe: also the azsp_rng_probe output (noise, uniforms) of the engine once the rounds are done."""
    b, dev = eu.backend(kind)
    eng = Engine(b, EngineConfig(game="go", board_size=5, num_games=STREAM_G, num_parallel=STREAM_P, num_simulations=200, seed=seed, rank=rank,
                                 leaf_symmetry=mode), device=dev)
    eng.reset_games()
    eng.priors.fill_(1.0 / eng.A)
    eng.select()
    out = []
    for _ in range(rounds):
        rows = np.flatnonzero(eng.valid.cpu().numpy())
        out.append((rows, eng.leaf_symmetries().cpu().numpy()[rows]))
        eng.round()
    pr = None
    if probe:
        import ctypes as C

        noise, unif = np.zeros((STREAM_G, 3, eng.A)), np.zeros((STREAM_G, 3, 4))
        assert b.dll.azsp_rng_probe(eng.h, 3, 4, noise.ctypes.data_as(C.c_void_p), unif.ctypes.data_as(C.c_void_p), None) == 0
        pr = (noise, unif)
    cnt = eng.counters()
    eng.close()
    return out, pr, cnt


def sym_draw(seed, rank, slot, count):
    """floor(8 u) of the leaf-symmetry stream: Philox4x32-10 keyed seed + rank, counters (slot, rows written so far, 0xFFD, 0x3000)."""
    r = philox4x32_10(seed + rank, slot, count, 0xFFD, 0x3000)
    return int((((r[0] << 32) | r[1]) >> 11) * (1.0 / 9007199254740992.0) * 8.0)


STREAM_SEED, STREAM_ROUNDS = 77, 18  # 40 root rows, then up to 320 leaf rows per round: more than 4000 rows, no move ends (26 rounds)


@functools.lru_cache(maxsize=None)
def stream_ops(kind, seed=STREAM_SEED, rank=2, rounds=STREAM_ROUNDS):
    return _uniform_rounds(kind, rounds, seed, rank, probe=True)


def check_stream(kind):
    """Every op is the draw recomputed here from an independent Philox with the slot's own row count as counter -- so rows of one game
    within a round are separate draws; same seed, same ops; another seed or rank, other ops; seed + rank is the key; the counts of
    the eight ops over N >= 4000 rows lie within N / 8 +- 5 sqrt(N * 7 / 64) (five standard deviations of a Binomial(N, 1/8));
    azsp_rng_probe and the search itself are what they are with the mode off."""
    rounds, probe, cnt = stream_ops(kind)
    count = np.zeros(STREAM_G, dtype=np.int64)
    all_ops, several = [], 0
    for rows, ops in rounds:
        for r, op in zip(rows, ops):
            g = int(r) // STREAM_P
            assert op == sym_draw(STREAM_SEED, 2, g, int(count[g])), (g, int(count[g]), int(op))
            count[g] += 1
        for g in np.unique(rows // STREAM_P):
            several += len(np.unique(ops[rows // STREAM_P == g])) > 1
        all_ops.append(ops)
    ops = np.concatenate(all_ops)
    N = len(ops)
    assert N >= 4000 and several > 100
    hist = np.bincount(ops, minlength=8)
    assert len(hist) == 8 and np.all(np.abs(hist - N / 8) <= 5 * np.sqrt(N * 7 / 64)), (N, hist.tolist())
    flat = lambda rs: np.concatenate([o for _, o in rs])  # noqa: E731
    again = _uniform_rounds(kind, 4, STREAM_SEED, 2)[0]
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(again, rounds))
    other_seed, other_rank = flat(_uniform_rounds(kind, 4, STREAM_SEED + 1, 2)[0]), flat(_uniform_rounds(kind, 4, STREAM_SEED, 3)[0])
    first = flat(rounds[:4])
    assert not np.array_equal(other_seed, first) and not np.array_equal(other_rank, first)
    assert np.array_equal(flat(_uniform_rounds(kind, 4, STREAM_SEED - 1, 3)[0]), first)  # the key is seed + rank
    # uniform priors and zero values are invariant under every op: the search, its other random streams and its counters do not move
    off_rounds, off_probe, off_cnt = _uniform_rounds(kind, STREAM_ROUNDS, STREAM_SEED, 2, mode=None, probe=True)
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(off_rounds, rounds)) and not flat(off_rounds).any()
    assert np.array_equal(off_probe[0], probe[0]) and np.array_equal(off_probe[1], probe[1]) and off_cnt == cnt


# ---------------------------------------------------------------------------------------------------
# 4. identity and off
# ---------------------------------------------------------------------------------------------------
def check_identity_and_off(kind, shape="go5"):
    """Fixed op 0 is the mode off; an engine that searched under symmetries and turned them off equals one that never did."""
    plain, plain_feats = _plain_run(kind, shape, None)
    got, feats = _run(kind, shape, eval_batch, feature_dtype=_abi.FEAT_I8, leaf_symmetry=0)
    assert_same_outputs(got, plain, "op 0")
    assert all(np.array_equal(f, g) for f, g in zip(feats, plain_feats))
    # used, then off: games under "random" (uniform priors: no evaluator in the loop), then the same engine plays the injected games
    b, dev = eu.backend(kind)
    noise, unif = _randomness(shape)
    G, M, A = noise.shape
    logs = {}
    for used in (False, True):
        eng = Engine(b, EngineConfig(num_games=G, inject_random=True, inject_moves=M, stop_at_game_end=True, log_moves=True, log_capacity=M,
                                     **SHAPES[shape]["kw"]), device=dev)
        eng.set_injection(noise, unif)
        if used:
            eng.set_leaf_symmetry("random")
            eng.reset_games()
            eng.priors.fill_(1.0 / A)
            eng.select()
            for _ in range(12):
                eng.round()
            assert eng.leaf_symmetries().any()
            eng.set_leaf_symmetry(None)
        eng.reset_games()
        eng.counters(reset=True)
        eng.select()
        for _ in range(100000):
            valid = eng.valid.cpu().numpy().astype(bool)
            st, _ = eng.status()
            if not valid.any() and np.all(st[:, _abi.STC_STATUS] == _abi.ST_IDLE):
                break
            assert not eng.leaf_symmetries().any()
            pri, val = np.zeros((eng.rows, A), np.float32), np.zeros(eng.rows, np.float32)
            rows = np.flatnonzero(valid)
            if len(rows):
                pri[rows], val[rows] = eval_batch(eu.decode_features(eng)[rows], A)
            eng.priors.copy_(torch.from_numpy(pri))
            eng.values.copy_(torch.from_numpy(val))
            eng.round()
        logs[used] = ([[tuple(x.tobytes() for x in eng.get_search(g, k)) for k in range(int(st[g, _abi.STC_PLY]))] for g in range(G)],
                      eng.counters())
        eng.close()
    assert logs[True] == logs[False] and all(len(g) > 0 for g in logs[False][0])
    assert [[x[0] for x in g] for g in logs[False][0]] == [[m["pi"].tobytes() for m in g] for g in plain.logs]


def check_resident_identity_gpu():
    """BatchSearch behind a DeviceEvaluator on a small 9x9 fp32-class (split-precision) network, the resident loop: op 0 is the plain
    search, bit for bit.  (Device only: the evaluator's kernels.)"""
    inf, ev = eu.small_go9_device_evaluator()
    assert "split-precision" in inf.evaluator_path(9, "cuda")
    boards, hist, pos = bc.positions("go", 9, 8, 6)
    rows = {}
    for mode in (None, 0, 3):
        bs = BatchSearch("go", 9, 6, 48, num_parallel=4, leaf_symmetry=mode)
        assert np.all(bs.load(boards, hist, pos) == _abi.SS_OK)
        bs.search(ev)
        rows[mode] = tuple(x.tobytes() for x in bs.results().cpu())
        bs.close()
    assert rows[0] == rows[None]
    assert rows[3] != rows[None]  # a ResNet is not equivariant: the op reaches the evaluator
    assert inf.split_range_status(reset=True)[0] == 0


# ---------------------------------------------------------------------------------------------------
# 5. public surfaces
# ---------------------------------------------------------------------------------------------------
def _search_rows(bs, ef):
    bs.search(ef)
    return tuple(x.tobytes() for x in bs.results().cpu())


def check_batch_search(kind, game="go", n=5, P=1):
    """BatchSearch(leaf_symmetry=k) with a host eval_func equals the plain BatchSearch with the wrapped function, on 8 positions and
    32 simulations; "random" runs and differs from none of the contracts (pi sums to 1)."""
    A = eu.num_actions(game, n)
    b, dev = eu.backend(kind)
    boards, hist, pos = bc.positions(game, n, 8, 8)
    ef = make_eval_func(A)

    def wrapped(k):
        w = wrapped_eval(k, n)

        def f(obs, batched=False):
            assert batched
            p, v = w(np.asarray(obs), A)
            return list(p), list(v)

        return f

    def make(mode):
        bs = BatchSearch(game, n, 8, 32, num_parallel=P, binding=b, device=dev, leaf_symmetry=mode)
        assert np.all(bs.load(boards, hist, pos) == _abi.SS_OK)
        return bs

    base = make(None)
    plain_rows = _search_rows(base, ef)
    base.close()
    for k in (0, 1, 3, 5, 6):
        sym, plain = make(k), make(None)
        got, want = _search_rows(sym, ef), _search_rows(plain, wrapped(k))
        assert got == want, k
        assert (got == plain_rows) == (k == 0), k
        sym.close(), plain.close()
    rnd = make("random")
    rnd.search(ef)
    pi, cn, _ = rnd.results().cpu()
    assert np.allclose(pi.sum(1), 1.0) and rnd.eng.leaf_symmetries().cpu().numpy().max() <= 7 and (cn.sum(1) >= 31).all()
    rnd.close()


def check_actor_random(kind, P=4):
    """SelfPlayActor(leaf_symmetry="random") plays and harvests whole 5x5 games: every pi row sums to 1, the harvested states are the
    true orientation (each game's samples replay: a sample's stone planes are the next sample's history), no range event."""
    import budget_checks as bk

    b, dev = eu.backend(kind)
    net = AlphaZeroNet((17, 5, 5), 26, 1, 8, 8)
    G = 8
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        actor = SynthActor(net, game="go", board_size=5, num_games=G, num_simulations=24, num_parallel=P, warm_up_steps=4, seed=5, device=dev,
                           net_dtype=torch.float32, use_graph=False, binding=b, tiled_features=False,
                           engine_kw=dict(stop_at_game_end=True, max_steps=bk.MAX_STEPS), leaf_symmetry="random")
    assert actor.engine.cfg.leaf_symmetry == "random"
    seen = []
    for _ in range(400):
        actor.run_rounds(4)
        seen.append(actor.engine.leaf_symmetries().cpu().numpy())
        if np.all(actor.engine.status()[0][:, _abi.STC_STATUS] == _abi.ST_IDLE):
            break
    else:
        raise AssertionError("the games did not finish")
    assert len(np.unique(np.concatenate(seen))) >= 4
    assert actor.range_events == 0  # (what bench.py reports as evaluator_range_events)
    states, pi, z, games, moves = (x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in actor.engine.harvest(sample_capacity=G * bk.MAX_STEPS, with_moves=True))
    assert len(games) == G and np.allclose(pi.sum(1), 1.0, atol=1e-6)
    eu.assert_game_samples(games, states, z, bk.MAX_STEPS)
    for row in games:
        st, pp, mv = eu.samples_of(row, states, pi, moves)
        assert not st[0, :16].any()  # a game starts on the empty board, whatever symmetry its root was evaluated under
        for k in range(len(st)):
            where = (int(row[_abi.GR_SLOT]), k)
            occupied = (st[k, 0] | st[k, 1]).reshape(-1).astype(bool)
            assert not pp[k, :25][occupied].any(), where  # pi lies on the sample's own board: no mass on a stone
            assert pp[k, mv[k]] > 0, where                # ... and the move that was played came out of it
            if k + 1 < len(st):  # the next sample shows this one's boards one step back, unrotated, plus the stone just played
                assert np.array_equal(st[k + 1, 3], st[k, 0]) and np.array_equal(st[k + 1, 2], st[k, 1]), where
                assert mv[k] == 25 or (st[k + 1, 1].reshape(-1)[mv[k]] == 1 and not occupied[mv[k]]), where


def check_refusals(kind):
    """Bad modes are AZSP_EINVAL at the ABI and ValueError, naming the allowed values, in Python."""
    b, dev = eu.backend(kind)
    eng = Engine(b, EngineConfig(game="go", board_size=5, num_games=2, num_parallel=2, num_simulations=8), device=dev)
    sym = lambda m: b.dll.azsp_set_leaf_symmetry(eng.h, m)  # noqa: E731
    assert [sym(8), sym(-3), sym(100), sym(-100)] == [-1] * 4
    assert [sym(m) for m in (_abi.SYM_OFF, _abi.SYM_RANDOM, 0, 7)] == [0] * 4
    assert b.dll.azsp_leaf_symmetries(eng.h, None, None) == -1 and b.dll.azsp_set_leaf_symmetry(None, 0) == -1
    for bad in (8, -1, "rot90", 1.0, True, "RANDOM", [3]):
        with pytest.raises(ValueError, match=r'None \(off\), "random" or an integer op 0\.\.7'):
            eng.set_leaf_symmetry(bad)
        with pytest.raises(ValueError, match="leaf_symmetry"):
            Engine(b, EngineConfig(game="go", board_size=5, num_games=1, num_parallel=1, num_simulations=4, leaf_symmetry=bad), device=dev)
        with pytest.raises(ValueError, match="leaf_symmetry"):
            BatchSearch("go", 5, 2, 8, binding=b, device=dev, leaf_symmetry=bad)
    net = AlphaZeroNet((17, 5, 5), 26, 1, 8, 8)
    with pytest.raises(ValueError, match="leaf_symmetry"):
        SynthActor(net, game="go", board_size=5, num_games=2, num_simulations=8, num_parallel=2, device=dev, binding=b, use_graph=False,
                   tiled_features=False, leaf_symmetry=9)
    eng.set_leaf_symmetry(np.int64(5))
    eng.set_leaf_symmetry("random")
    eng.set_leaf_symmetry(None)
    assert not eng.leaf_symmetries().any()
    eng.close()
