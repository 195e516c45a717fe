"""Shared drivers of policy surprise weighting (azsp_set_policy_surprise / azsp_harvest_surprise / azsp_replay_add_weighted:
EngineConfig.policy_surprise, Engine.harvest(with_surprise=True), SelfPlayActor(policy_surprise=), DeviceReplay.add_harvest(weights=)).
The same functions run on the host twin (CPU tier) and on the device (`-m gpu`).

The yardsticks are restated here in NumPy, not taken from the engine.

Surprise.  KL = sum over pi(a) > 0 of pi(a) (log pi(a) - log max(P(a), 1e-45)) + log Z in float64, P = the synthetic evaluator's float32
prior row of the harvested state, Z its mass on the actions the oracle env calls legal after replaying the harvested moves.  The engine
and NumPy differ in their logs and in the order of their sums, so the comparison has a tolerance, derived here and never measured.
With u = 2^-53 and every |log| < 128 (asserted: pi(a) > 1e-55 wherever it is positive; P is floored at 1e-45):
  a log is within 1 ulp <= 2^-46 = 128 u of the true value in either implementation; d = log pi - log P, |d| < 256, adds a rounding
  of 128 u: 384 u on d; the product pi(a) d adds u |pi(a) d| <= 256 u pi(a): 640 u pi(a) per term, 640 u over a row (sum pi = 1; 1024 u is
  taken, which covers a float32 row's sum being 1 only to 2^-24 A);
  summing A terms in any order costs at most A u sum |term| <= 256 A u;
  Z carries a relative error <= A u from its own sum, so log Z an absolute one <= A u, plus its ulp <= 128 u, plus 128 u for the last
  addition (|KL| < 256).
Per implementation (1024 + 256 + 257 A) u < (1536 + 257 A) u; the two together TOL64(A) = 2 (1536 + 257 A) 2^-53 (2.1e-11 at A = 362).
The staged value is the engine's KL rounded to float32: half a float32 ulp of the value is added.  Where the restatement takes pi from
the harvested float32 row instead of its float64 source (forced playouts, Gumbel: the move log holds the unpruned policy), each pi(a) is
off by at most max(2^-24 pi(a), 2^-150) and d KL / d pi(a) = log pi(a) + 1 - log P(a) is below 257 in magnitude: TOL_PI32(A) =
257 (2^-24 + A 2^-150) is added (1.6e-5).

Weights.  The formula of include/azsp.h on the harvested float32 surprises and class bytes in float64, in the same operation order:
exact.  Replay.  np.repeat of the rows by c_i = floor(w_i) + (u_i < w_i - floor(w_i)), then the ring write of add_samples: exact."""
import numpy as np
import pytest
import torch

import engine_util as eu
from alpha_zero_amd import _abi
from alpha_zero_amd.core.engine import Engine, EngineConfig, policy_surprise_params
from alpha_zero_amd.core.replay import DeviceReplay
from aux_checks import _actor, _finish, _drain_games
from synth_eval import eval_batch

G, P, KOMI, EINVAL = 8, 2, 7.5, -1
U = 2.0 ** -53


def tol64(A):
    return 2.0 * (1536 + 257 * A) * U


def tol_pi32(A):
    return 257.0 * (2.0 ** -24 + A * 2.0 ** -150)


# ---------------------------------------------------------------------------------------------------
# the restatements
# ---------------------------------------------------------------------------------------------------
def restated_kl(pi, prior, legal):
    """pi float64[A] (or float32, widened), prior float32[A], legal bool[A] -> KL in float64, before the clamp at 0."""
    pi, p = np.asarray(pi, dtype=np.float64), np.asarray(prior, dtype=np.float32).astype(np.float64)
    z = p[np.asarray(legal, dtype=bool)].sum()
    m = pi > 0
    assert pi[m].min() > 1e-55  # (every |log| < 128: the tolerance's premise)
    kl = float(np.sum(pi[m] * (np.log(pi[m]) - np.log(np.maximum(p[m], 1e-45)))))
    return kl + (float(np.log(z)) if z > 0 else 0.0)


def restated_weights(surprise, full, frac, include_fast):
    """One game's float32 surprises and class bytes -> float32 weights: the header's formula in float64, in its operation order."""
    f, nf, s = np.float64(frac), np.float64(0.0), np.float64(0.0)
    for sk, fk in zip(surprise, full):
        if fk:
            nf = nf + np.float64(1.0)
        if fk or include_fast:
            s = s + np.float64(sk)  # sequential, in row order
    out = np.zeros(len(surprise), dtype=np.float32)
    for k, (sk, fk) in enumerate(zip(surprise, full)):
        fk64 = np.float64(1.0 if fk else 0.0)
        if not s > 0:
            out[k] = np.float32(fk64)
            continue
        share = f * nf * np.float64(sk) / s if (fk or include_fast) else np.float64(0.0)
        out[k] = np.float32((np.float64(1.0) - f) * fk64 + share)
    return out


def restated_copies(weights, unif):
    w = np.asarray(weights, dtype=np.float32).astype(np.float64)
    w = np.where(w > 0, np.minimum(w, 2.0 ** 20), 0.0)  # (a NaN compares false: 0)
    fl = np.floor(w)
    return (fl + (np.asarray(unif, dtype=np.float64) < w - fl)).astype(np.int64)


def check_restatements():
    """The yardsticks on values known by hand."""
    p = np.array([0.5, 0.25, 0.25, 0.0], np.float32)
    assert restated_kl([0.5, 0.25, 0.25, 0.0], p, [1, 1, 1, 1]) == 0.0
    # an illegal action's prior mass is taken out: pi = P / Z on the legal ones is no surprise either
    assert abs(restated_kl([2 / 3, 1 / 3, 0, 0], p, [1, 1, 0, 0])) < 1e-15
    assert abs(restated_kl([1.0, 0, 0, 0], p, [1, 1, 1, 1]) - np.log(2.0)) < 1e-15
    assert restated_kl([0, 0, 0, 1.0], p, [1, 1, 1, 1]) == pytest.approx(-np.log(1e-45))  # the floor
    w = restated_weights(np.array([1.0, 3.0, 9.0], np.float32), [1, 1, 0], 0.5, False)
    assert w.tolist() == [0.75, 1.25, 0.0]
    w = restated_weights(np.array([1.0, 3.0, 4.0], np.float32), [1, 1, 0], 0.5, True)
    assert w.tolist() == [0.625, 0.875, 0.5]
    assert restated_weights(np.zeros(3, np.float32), [1, 0, 1], 0.5, True).tolist() == [1.0, 0.0, 1.0]
    assert restated_copies([0.0, 2.0, 2.5, 2.5, np.nan, -1.0, 1e30], [0.0, 0.99, 0.49, 0.5, 0.0, 0.0, 0.5]).tolist() == [0, 2, 3, 2, 0, 0, 2 ** 20]


# ---------------------------------------------------------------------------------------------------
# engines that play by themselves on a synthetic evaluator
# ---------------------------------------------------------------------------------------------------
def make_engine(kind, game="go", n=5, surprise=0.5, sims=8, seed=7, num_games=G, playout_cap=None, prune=True, parallel=P, **kw):
    b, dev = eu.backend(kind)
    kw.setdefault("stop_at_game_end", True)
    eng = Engine(b, EngineConfig(game=game, board_size=n, num_games=num_games, num_parallel=parallel, num_simulations=sims, warm_up_steps=4, komi=KOMI,
                                 seed=seed, policy_surprise=surprise, **kw), device=dev, playout_cap=playout_cap, prune_policy_target=prune)
    eng.reset_games()
    return eng


def play(eng, done=_abi.ST_IDLE, limit=20000, evaluator=eval_batch):
    """select -> evaluator on the valid rows -> round, until every slot's status is `done`."""
    eng.select()
    for _ in range(limit):
        valid = eng.valid.cpu().numpy().astype(bool)
        if not valid.any() and np.all(eng.status()[0][:, _abi.STC_STATUS] == done):
            return
        rows = np.flatnonzero(valid)
        pri, val = np.zeros((eng.rows, eng.A), np.float32), np.zeros(eng.rows, np.float32)
        if len(rows):
            pri[rows], val[rows] = evaluator(eu.decode_features(eng)[rows], eng.A)
        eng.priors.copy_(torch.from_numpy(pri))
        eng.values.copy_(torch.from_numpy(val))
        eng.round()
    raise AssertionError("the games did not finish")


KEYS = ("states", "pi", "z", "games", "moves", "full")


def drain(eng, with_surprise=True, with_aux=False, **kw):
    """Every finished game: dict of host arrays (states, pi, z, games with START rebased, moves, full[, aux][, surprise, weight])."""
    keys = KEYS + (("ownership", "score", "root_q") if with_aux else ()) + (("surprise", "weight") if with_surprise else ())
    parts, base = [], 0
    while True:
        got = eng.harvest(with_moves=True, with_class=True, with_aux=with_aux, with_surprise=with_surprise, **kw)
        assert len(got) == len(keys)
        if len(got[3]) == 0:
            break
        games = got[3].copy()
        games[:, _abi.GR_START] += base
        base += len(got[2])
        parts.append([t.cpu().numpy().copy() if i != 3 else games for i, t in enumerate(got)])
    assert parts
    out = {k: np.concatenate([p[i] for p in parts]) for i, k in enumerate(keys)}
    if with_surprise:
        assert out["surprise"].dtype == out["weight"].dtype == np.float32 and out["surprise"].shape == out["weight"].shape == out["z"].shape
    return out


def legal_masks(game, n, moves, max_steps=0, num_to_win=5):
    """(legal bool[len, A], observations int8[len, 17, n, n]) in front of every harvested move of one game, from the CPU oracle's env."""
    env = eu.make_oracle_env(game, n, max_steps, num_to_win)
    env.reset()
    legal, obs = [], []
    for m in moves:
        legal.append(np.asarray(env.legal_actions) != 0)
        obs.append(np.asarray(env.observation(), dtype=np.int8).copy())
        if m >= 0:
            env.step(int(m))
    return np.stack(legal), np.stack(obs)


# ---------------------------------------------------------------------------------------------------
# 1. surprise against the restatement
# ---------------------------------------------------------------------------------------------------
SHAPES = {("go", 5): dict(max_steps=14), ("go", 9): dict(max_steps=16), ("go", 19): dict(max_steps=6), ("gomoku", 7): dict(num_to_win=4)}
VARIANTS = {"plain": dict(root_noise=False), "noise": dict(root_noise=True), "forced": dict(forced_playouts=2), "gumbel": dict(gumbel=4)}


def check_surprise(kind, game, n, variant="plain"):
    """Every harvested surprise is float32(max(KL, 0)) of the restatement within the derived tolerance.  pi is the float64 row of the move
    log where the sample records the plain policy (asserted: its float32 rounding is the harvested row), else the harvested row.  The
    harvest holds a row with surprise > 0.1 and rows on a kept sub-tree (reuse_tree, ply > 0); with Dirichlet noise the prior is still
    the raw one (the restatement knows no noise)."""
    shape = SHAPES[(game, n)]
    cap = shape.get("max_steps", n * n)
    from_log = variant in ("plain", "noise")
    eng = make_engine(kind, game, n, reuse_tree=True, log_moves=True, log_capacity=cap, **shape, **VARIANTS[variant])
    A = eng.A
    play(eng)
    logged = {(g, k): eng.get_search(g, k)[0].copy() for g in range(G) for k in range(cap)} if from_log else {}
    h = drain(eng)
    eng.close()
    assert len(h["games"]) == G
    tol = tol64(A) + (0.0 if from_log else tol_pi32(A))
    kept = worst = 0
    for row in h["games"]:
        st, pi32, mv, got = eu.samples_of(row, h["states"], h["pi"], h["moves"], h["surprise"])
        legal, obs = legal_masks(game, n, mv, shape.get("max_steps", 0), shape.get("num_to_win", 5))
        assert np.array_equal(obs, st)  # the replayed positions are the harvested ones
        prior = eval_batch(st, A)[0]
        for k in range(len(mv)):
            where = (variant, int(row[_abi.GR_SLOT]), k)
            pi = logged[(int(row[_abi.GR_SLOT]), k)] if from_log else pi32[k]
            if from_log:
                assert np.array_equal(pi.astype(np.float32), pi32[k]), where  # the float64 source of the harvested row
            assert not np.any((pi > 0) & ~legal[k]), where
            want = max(restated_kl(pi, prior[k], legal[k]), 0.0)
            err = abs(float(got[k]) - want)
            bound = tol + 0.5 * float(np.spacing(np.float32(max(want, float(got[k])))))
            print(f"surprise {where}: got {float(got[k]):.9g} want {want:.17g} |diff| {err:.3g} bound {bound:.3g}")
            assert got[k] >= 0 and err <= bound, (where, float(got[k]), want, err, bound)
            kept += k > 0
            worst = max(worst, float(got[k]))
    assert worst > 0.1 and kept > 0
    assert len(set(h["surprise"].tolist())) > len(h["surprise"]) // 2  # (not a column of one constant)


# ---------------------------------------------------------------------------------------------------
# 2. weights, bit for bit
# ---------------------------------------------------------------------------------------------------
def assert_game_weights(h, row, frac, include_fast):
    s, full, w = eu.samples_of(row, h["surprise"], h["full"], h["weight"])
    want = restated_weights(s, full, frac, include_fast)
    assert w.tobytes() == want.tobytes(), (int(row[_abi.GR_SLOT]), w, want)
    nf = int(np.count_nonzero(full))
    total = float(np.sum(w.astype(np.float64)))
    assert abs(total - nf) <= len(w) * float(np.spacing(np.float32(max(nf, 1)))), (total, nf)  # sum = Nf within len float32 ulps
    return s, full, w


def check_weights(kind, frac, include_fast, n=5, max_steps=14):
    """Under a playout cap (2 fast simulations, half the moves full) the harvested weights are the restated formula on the harvested
    surprises and class bytes, bit for bit; each game's weights sum to its number of full rows.  Some game has both classes; for
    frac > 0 some row outweighs 1, some full row falls below 1 and, with include_fast, some fast row earns a share; frac = 0 gives
    weight == full."""
    eng = make_engine(kind, "go", n, surprise=(frac, include_fast), playout_cap=(2, 0.5), max_steps=max_steps)
    play(eng)
    h = drain(eng)
    eng.close()
    assert len(h["games"]) == G
    both = False
    for row in h["games"]:
        s, full, w = assert_game_weights(h, row, frac, include_fast)
        both = both or (full.any() and not full.all())
    full, w = h["full"] != 0, h["weight"]
    assert both and np.any(h["surprise"][~full] > 0)  # (fast moves carry a surprise too, whoever takes part)
    if frac == 0:
        assert np.array_equal(w, full.astype(np.float32))
    else:
        assert np.any(w > 1) and np.any(w[full] < 1)
        assert np.any(w[~full] > 0) if include_fast else not np.any(w[~full])


def one_hot_evaluator(obs_batch, num_actions):
    """The prior is 1.0 on the first empty point (no stone on the two newest planes) and 0.0 elsewhere, the value 0."""
    pri = np.zeros((len(obs_batch), num_actions), np.float32)
    for i, o in enumerate(obs_batch):
        pri[i, int(np.flatnonzero((o[0] == 0).ravel() & (o[1] == 0).ravel())[0])] = 1.0
    return pri, np.zeros(len(obs_batch), np.float32)


def check_zero_surprise_game(kind, n=7):
    """Gomoku on an evaluator whose prior is a one-hot on a legal point: the one simulation of every search (2 with the root's own, one leaf per
    round) must visit it, the target is that one-hot, KL = 1 (log 1 - log 1) + log 1 = 0 exactly -- and a game without surprise is weighted uniformly."""
    eng = make_engine(kind, "gomoku", n, surprise=1.0, sims=2, num_to_win=4, root_noise=False, parallel=1)
    play(eng, evaluator=one_hot_evaluator)
    h = drain(eng)
    eng.close()
    assert len(h["games"]) == G and len(h["z"]) >= 4 * G
    assert np.all(h["pi"].max(axis=1) == 1.0)
    assert not h["surprise"].any() and np.all(h["weight"] == 1.0)


def check_both_staging_buffers(kind, n=5, max_steps=6, frac=0.5):
    """aux_checks.check_both_staging_buffers' stall: without a harvest every slot fills both of its staging buffers; one harvest hands out
    two games per slot, each weighted by its own sum."""
    eng = make_engine(kind, "go", n, surprise=frac, max_steps=max_steps, stop_at_game_end=False)
    play(eng, done=_abi.ST_WAIT_BUF)
    h = drain(eng, sample_capacity=2 * G * max_steps, max_games=2 * G)
    eng.close()
    assert len(h["games"]) == 2 * G
    sums = {}
    for row in h["games"]:
        s, _, w = assert_game_weights(h, row, frac, False)
        sums.setdefault(int(row[_abi.GR_SLOT]), []).append(float(np.sum(s.astype(np.float64))))
    assert sorted(sums) == list(range(G)) and all(len(v) == 2 for v in sums.values())
    assert all(a != b for a, b in sums.values())  # the two buffers of a slot hold different sums: a shared one would miss the exact weights


# ---------------------------------------------------------------------------------------------------
# 3. off is off
# ---------------------------------------------------------------------------------------------------
def check_off_is_off(kind, n=5, max_steps=14):
    """Same seed with and without the feature (aux targets on in both): states, pi, z, game rows, moves, classes, counters and the three
    aux outputs are identical.  The refusals.  Turned off again: surprises harvested as 0, weights = full."""
    b, dev = eu.backend(kind)
    kw = dict(max_steps=max_steps, aux_targets=True, playout_cap=(2, 0.5))
    on, off = (make_engine(kind, "go", n, surprise=s, **kw) for s in ((0.5, True), None))
    assert on.policy_surprise and not off.policy_surprise
    assert b.dll.azsp_harvest_surprise(off.h, None, None) == 0
    buf = torch.zeros(4 * G * max_steps, dtype=torch.float32, device=dev)
    for args in ((buf.data_ptr(), None), (None, buf.data_ptr())):
        assert b.dll.azsp_harvest_surprise(off.h, *args) == EINVAL  # never enabled: nothing is staged
    with pytest.raises(_abi.AzspError):
        off.harvest(with_surprise=True)
    for frac in (-0.01, 1.01, float("nan")):
        assert b.dll.azsp_set_policy_surprise(on.h, 1, frac, 0) == EINVAL
    for bad in (-0.1, 1.5, "x", (0.5, 1), (0.5, True, 1), True):
        with pytest.raises(ValueError, match="policy_surprise"):
            policy_surprise_params(bad)
    assert policy_surprise_params(None) == (0, 0.0, 0) and policy_surprise_params(1) == (1, 1.0, 0) and policy_surprise_params((0.25, True)) == (1, 0.25, 1)
    play(on), play(off)
    assert on.counters() == off.counters()
    hon, hoff = drain(on, with_aux=True), drain(off, with_surprise=False, with_aux=True)
    for key in KEYS + ("ownership", "score", "root_q"):
        assert hon[key].tobytes() == hoff[key].tobytes() and hon[key].shape == hoff[key].shape, key
    assert hon["surprise"].any()
    on.close(), off.close()
    # a drop-in engine records no samples
    drop = Engine(b, EngineConfig(game="go", board_size=n, num_games=2, num_parallel=1, num_simulations=4, stop_after_move=True), device=dev)
    assert b.dll.azsp_set_policy_surprise(drop.h, 1, 0.5, 0) == EINVAL and b.dll.azsp_set_policy_surprise(drop.h, 0, 0.5, 0) == EINVAL
    drop.close()
    with pytest.raises(_abi.AzspError):
        Engine(b, EngineConfig(game="go", board_size=n, num_games=2, num_parallel=1, num_simulations=4, stop_after_move=True, policy_surprise=0.5), device=dev)
    # on, then off again before the first move: the row exists, every move stages 0, every game is weighted `full`
    eng = make_engine(kind, "go", n, surprise=(0.5, True), max_steps=max_steps, playout_cap=(2, 0.5))
    eng.set_policy_surprise(None)
    play(eng)
    h = drain(eng)
    eng.close()
    assert not h["surprise"].any() and np.array_equal(h["weight"], (h["full"] != 0).astype(np.float32)) and not h["full"].all()
    for key in ("states", "pi", "z", "moves", "full"):
        assert h[key].tobytes() == hon[key].tobytes(), key
    # one output at a time
    eng = make_engine(kind, "go", n, surprise=0.5, max_steps=max_steps)
    play(eng)
    cap = 2 * max_steps
    outs = [torch.full((cap,), 77.0, dtype=torch.float32, device=dev) for _ in range(2)]
    for only in (0, 1):
        for t in outs:
            t.fill_(77)
        assert b.dll.azsp_harvest_surprise(eng.h, *[t.data_ptr() if i == only else None for i, t in enumerate(outs)]) == 0
        games = eng.harvest(sample_capacity=cap, max_games=2)[3]  # (a harvest without with_surprise leaves the pointers set above alone)
        total = int(games[:, _abi.GR_LENGTH].sum())
        assert len(games) == 2 and np.all(outs[1 - only].cpu().numpy() == 77)
        got = outs[only].cpu().numpy()
        assert np.all(got[:total] != 77) and np.all(got[total:] == 77) and np.all(got[:total] >= 0)
    eng.close()


# ---------------------------------------------------------------------------------------------------
# 4. weighted add, exact against NumPy
# ---------------------------------------------------------------------------------------------------
AUX_KEYS = ("ownership", "score", "root_q")


def _samples(rng, n, A, count, dev):
    return dict(states=torch.from_numpy(rng.integers(0, 2, size=(count, 17, n, n)).astype(np.int8)).to(dev),
                pi=torch.from_numpy(rng.random((count, A)).astype(np.float32)).to(dev),
                z=torch.from_numpy(rng.choice([-1.0, 0.0, 1.0], size=count).astype(np.float32)).to(dev),
                ownership=torch.from_numpy(rng.integers(-1, 2, size=(count, n, n)).astype(np.int8)).to(dev),
                score=torch.from_numpy((rng.integers(-60, 60, size=count) + 0.5).astype(np.float32)).to(dev),
                root_q=torch.from_numpy(rng.uniform(-1, 1, size=count).astype(np.float32)).to(dev))


class RingModel:
    """The ring as the reference's per-transition loop leaves it after appending np.repeat(rows, c)."""

    def __init__(self, cap, sample, keys, seed):
        self.cap, self.added, self.rs = cap, 0, np.random.RandomState(seed)
        self.ring = {k: np.zeros((cap,) + tuple(sample[k].shape[1:]), dtype=sample[k].cpu().numpy().dtype) for k in keys}

    def add(self, s, weights):
        count = len(weights)
        c = restated_copies(weights, self.rs.random_sample(count))  # one uniform per row, in row order
        rep = np.repeat(np.arange(count), c)
        skip = max(0, len(rep) - self.cap)
        for j, i in enumerate(rep[skip:]):
            for k, ring in self.ring.items():
                ring[(self.added + skip + j) % self.cap] = s[k].cpu().numpy()[i]
        self.added += len(rep)
        return c


def _rings(rep, keys):
    return {k: getattr(rep, k).cpu().numpy() for k in keys}


def _add(rep, s, weights, aux, games=1):
    rep.add_samples(s["states"], s["pi"], s["z"], num_games=games, aux=tuple(s[k] for k in AUX_KEYS) if aux else None, weights=weights)


def check_weighted_add(kind, n, aux):
    """Every case of the issue against RingModel with the same RandomState: empty and single adds, the special weights, more rows than
    one scan chunk, more copies than the ring holds, a wrap, two adds in a row; then sample_device reads rows of the restated ring."""
    b, dev = eu.backend(kind)
    A = n * n + 1
    keys = ("states", "pi", "z") + (AUX_KEYS if aux else ())
    rng = np.random.Generator(np.random.PCG64(11 + n))

    def pair(cap, seed, like):
        return (DeviceReplay(cap, np.random.RandomState(seed), n, A, device=dev, binding=b, aux_targets=aux), RingModel(cap, like, keys, seed))

    def same(rep, model):
        for k, ring in _rings(rep, keys).items():
            assert ring.tobytes() == model.ring[k].tobytes(), k
        assert rep.num_samples_added == model.added

    # n = 0, n = 1, the special weights, a second add that wraps the ring end
    s = _samples(rng, n, A, 9, dev)
    rep, model = pair(13, 3, s)
    empty = {k: v[:0] for k, v in s.items()}
    _add(rep, empty, torch.zeros(0), aux)
    model.add(empty, np.zeros(0, np.float32))
    same(rep, model)
    assert (rep.num_samples_added, rep.num_games_added) == (0, 1)
    one = {k: v[:1] for k, v in s.items()}
    _add(rep, one, torch.tensor([1.0]), aux)
    assert model.add(one, np.float32([1.0])).tolist() == [1]
    same(rep, model)
    w = np.array([0.0, 1.0, 3.0, 0.5, 0.5, 1.75, np.nan, -2.0, 0.25], np.float32)
    c = model.add(s, w)
    assert c[0] == 0 and c[1] == 1 and c[2] == 3 and c[6] == 0 and c[7] == 0 and 1 + c.sum() < 13
    _add(rep, s, torch.from_numpy(w).to(dev), aux, games=2)
    same(rep, model)
    w2 = rng.uniform(0, 2.5, size=9).astype(np.float32)
    c2 = model.add(s, w2)
    assert 1 + c.sum() + c2.sum() > 13 >= c2.sum()  # wraps the ring end without overflowing it
    _add(rep, s, w2, aux)  # (a host array works like a device tensor)
    same(rep, model)
    assert rep.num_games_added == 5 and rep.size == 13
    # total > capacity: only the last `capacity` copies, in order
    rep, model = pair(7, 4, s)
    w3 = np.array([2.0, 1.5, 0.0, 3.0, 1.0, 2.5, 1.0, 0.5, 2.0], np.float32)
    assert model.add(s, w3).sum() > 7
    _add(rep, s, w3, aux)
    same(rep, model)
    rep, model = pair(5, 5, s)
    assert model.add(one, np.float32([40.0])).tolist() == [40]  # one row, more copies than the ring holds
    _add(rep, one, np.float32([40.0]), aux)
    same(rep, model)
    assert np.all(rep.z.cpu().numpy() == one["z"].cpu().numpy()[0])
    # n = 1030: more than one scan chunk
    big = _samples(rng, n, A, 1030, dev)
    rep, model = pair(1500, 6, big)
    wb = rng.uniform(0, 2, size=1030).astype(np.float32)
    wb[::7] = np.float32(1.0)
    cb = model.add(big, wb)
    assert 900 < cb.sum() < 1500
    _add(rep, big, wb, aux)
    same(rep, model)
    # reads: sample_device returns rows of the restated ring
    size = rep.size
    rep.random_state = np.random.RandomState(21)
    idx = np.random.RandomState(21).randint(low=0, high=size, size=16)
    got = rep.sample_device(16, transform=0, with_aux=aux)
    assert np.array_equal(got[0].cpu().numpy(), model.ring["states"][idx].astype(np.float32))
    assert got[1].cpu().numpy().tobytes() == model.ring["pi"][idx].tobytes() and got[2].cpu().numpy().tobytes() == model.ring["z"][idx].tobytes()
    if aux:
        assert got[4].cpu().numpy().tobytes() == model.ring["score"][idx].tobytes()


def check_weighted_add_rules(kind, n=5):
    """weights = full as floats leaves the ring add_harvest(keep=full) leaves, byte for byte; weights with keep raises; the C entry
    refuses an aux ring without its source; a wrong number of weights raises."""
    b, dev = eu.backend(kind)
    A, cap, count = n * n + 1, 19, 23
    rng = np.random.Generator(np.random.PCG64(5))
    s = _samples(rng, n, A, count, dev)
    games = np.zeros((3, _abi.GR_COUNT), dtype=np.int32)
    full = torch.from_numpy(rng.random(count) < 0.6).to(dev)
    aux = tuple(s[k] for k in AUX_KEYS)
    keys = ("states", "pi", "z") + AUX_KEYS
    a, c = (DeviceReplay(cap, np.random.RandomState(1), n, A, device=dev, binding=b, aux_targets=True) for _ in range(2))
    for _ in range(2):  # the second round wraps
        a.add_harvest(s["states"], s["pi"], s["z"], games, keep=full, aux=aux)
        c.add_harvest(s["states"], s["pi"], s["z"], games, weights=full.to(torch.float32), aux=aux)
    assert 2 * int(full.sum()) > cap
    for k in keys:
        assert getattr(a, k).cpu().numpy().tobytes() == getattr(c, k).cpu().numpy().tobytes(), k
    assert (a.num_samples_added, a.num_games_added) == (c.num_samples_added, c.num_games_added) == (2 * int(full.sum()), 6)
    with pytest.raises(ValueError, match="keep"):
        c.add_harvest(s["states"], s["pi"], s["z"], games, keep=full, aux=aux, weights=full.to(torch.float32))
    with pytest.raises(ValueError, match="weight"):
        c.add_samples(s["states"], s["pi"], s["z"], aux=aux, weights=torch.ones(count - 1))
    with pytest.raises(ValueError, match="aux"):
        c.add_samples(s["states"], s["pi"], s["z"], weights=torch.ones(count))
    w, u = torch.ones(count, dtype=torch.float32, device=dev), torch.zeros(count, dtype=torch.float64, device=dev)
    ofs = torch.zeros(count + 1, dtype=torch.int32, device=dev)
    before = c.states.clone()
    rc = b.dll.azsp_replay_add_weighted(c.states.data_ptr(), c.pi.data_ptr(), c.z.data_ptr(), cap, 0, s["states"].data_ptr(), s["pi"].data_ptr(),
                                        s["z"].data_ptr(), count, 17, n, A, w.data_ptr(), u.data_ptr(), c.ownership.data_ptr(), None, None, None, None,
                                        None, ofs.data_ptr(), None)
    assert rc == EINVAL and torch.equal(before, c.states)
    rc = b.dll.azsp_replay_add_weighted(c.states.data_ptr(), c.pi.data_ptr(), c.z.data_ptr(), cap, 0, s["states"].data_ptr(), s["pi"].data_ptr(),
                                        s["z"].data_ptr(), count, 17, n, A, w.data_ptr(), u.data_ptr(), None, None, None, None, s["score"].data_ptr(),
                                        None, ofs.data_ptr(), None)
    assert rc == EINVAL and torch.equal(before, c.states)


# ---------------------------------------------------------------------------------------------------
# 5. the actor
# ---------------------------------------------------------------------------------------------------
def check_actor(kind, n=5, max_steps=12, surprise=(0.5, True), cap=(2, 0.5)):
    """SelfPlayActor(policy_surprise=, playout_cap=): harvest_tensors() keeps its 4-tuple and leaves one surprise and one weight per sample
    next to last_harvest_full, the rows Engine.harvest(with_surprise=True) of a twin actor returns and the restatement confirms; clones
    and views as for the aux rows; add_harvest(weights=, aux=) fills a replay; the reference-format harvest() is what it is without."""
    b, dev = eu.backend(kind)
    kw = dict(policy_surprise=surprise, playout_cap=cap, aux_targets=True)
    a, v, tw, ref, off = (_actor(kind, n, max_steps, **k) for k in (kw, kw, kw, kw, dict(playout_cap=cap, aux_targets=True)))
    assert a.policy_surprise and a.engine.policy_surprise and a.last_harvest_weight is None and not off.policy_surprise
    for x in (a, v, tw, ref, off):
        _finish(x)
    want = drain(tw.engine, with_aux=True)
    A = n * n + 1
    rep = DeviceReplay(64, np.random.RandomState(2), n, A, device=dev, binding=b, aux_targets=True)
    model = RingModel(64, {k: torch.from_numpy(want[k]) for k in ("states", "pi", "z") + AUX_KEYS}, ("states", "pi", "z") + AUX_KEYS, 2)
    for actor, clone in ((a, True), (v, False)):
        rows = {k: [] for k in ("z", "full", "surprise", "weight")}
        while True:
            got = actor.harvest_tensors(clone=clone)
            assert len(got) == 4  # the 4-tuple it always was
            if len(got[3]) == 0:
                break
            s, w = actor.last_harvest_surprise, actor.last_harvest_weight
            assert s.shape == w.shape == got[2].shape == actor.last_harvest_full.shape and s.dtype == w.dtype == torch.float32
            same = [t.data_ptr() == u.data_ptr() for t, u in zip((s, w), actor.engine._harvest_surprise_bufs)]
            assert not any(same) if clone else all(same)  # clone=True: private copies; else views of the engine's buffers like the rest
            if clone:  # the first actor's harvests go into the replay, fast moves included: their weight decides
                rep.add_harvest(*got, weights=w, aux=actor.last_harvest_aux)
                model.add(dict(zip(("states", "pi", "z") + AUX_KEYS, got[:3] + tuple(actor.last_harvest_aux))), w.cpu().numpy())
            for k, t in zip(rows, (got[2], actor.last_harvest_full, s, w)):
                rows[k].append(t.cpu().numpy().copy())
        for k in rows:
            assert np.concatenate(rows[k]).tobytes() == (want[k] != 0 if k == "full" else want[k]).tobytes(), (k, clone)
    for row in want["games"]:
        assert_game_weights(want, row, *surprise)
    assert want["surprise"].any() and np.any(want["weight"][want["full"] == 0] > 0)
    for k in ("states", "pi", "z") + AUX_KEYS:
        assert getattr(rep, k).cpu().numpy().tobytes() == model.ring[k].tobytes(), k
    assert rep.num_samples_added == model.added > 0 and rep.num_games_added == G
    gon, goff = _drain_games(ref), _drain_games(off)
    assert len(gon) == len(goff) == G
    for (s1, st1, m1), (s2, st2, m2) in zip(gon, goff):
        assert st1 == st2 and m1 == m2 and len(s1) == len(s2) > 0
        assert all(np.array_equal(t.state, u.state) and np.array_equal(t.pi_prob, u.pi_prob) and t.value == u.value for t, u in zip(s1, s2))
    assert off.harvest_tensors() is not None and off.last_harvest_weight is None and off.last_harvest_surprise is None
    with pytest.raises(ValueError, match="policy_surprise"):
        _actor(kind, n, max_steps, policy_surprise=0.5, engine_kw=dict(stop_after_move=True))
    with pytest.raises(ValueError, match="policy_surprise"):
        _actor(kind, n, max_steps, policy_surprise=1.5)
