"""Shared drivers for the engine parity tests.  The same functions run against
  * the host twin (tests/hosttwin, CPU, `-m "not gpu"`): identical engine source, WaveHost policy
  * libazsp.so on a MI355X (`-m gpu`): the product
and compare with the golden vectors produced by the reference / with the CPU oracle."""
import contextlib
import ctypes
import hashlib
import os
import subprocess
from types import SimpleNamespace
from typing import NamedTuple

import numpy as np
import torch

from alpha_zero_amd import _abi
from alpha_zero_amd.core.engine import Engine, EngineConfig

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_twin = None


_twin_variants = {}


def hosttwin_variant(tag, defines):
    """A host twin compiled with extra -D flags (e.g. a tiny AZ_PATH_CAP to exercise the deep-path fallback)."""
    if tag not in _twin_variants:
        src = os.path.join(HERE, "hosttwin", "azsp_host.cpp")
        so = os.path.join(HERE, "hosttwin", f"libazsp_hosttwin_{tag}.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-fno-strict-aliasing"] + defines + ["-o", so, src])
        _twin_variants[tag] = _abi.Binding(ctypes.CDLL(so), f"hosttwin_{tag}")
    return _twin_variants[tag]


def hosttwin_binding():
    """Builds (once) and loads the host twin -- test infrastructure, never used by the product."""
    global _twin
    if _twin is None:
        src = os.path.join(HERE, "hosttwin", "azsp_host.cpp")
        so = os.path.join(HERE, "hosttwin", "libazsp_hosttwin.so")
        deps = [src] + [os.path.join(ROOT, "alpha_zero_amd", "csrc", f) for f in os.listdir(os.path.join(ROOT, "alpha_zero_amd", "csrc"))
                        if f.endswith(".h")] + [os.path.join(ROOT, "include", "azsp.h")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-fno-strict-aliasing", "-o", so, src])
        _twin = _abi.Binding(ctypes.CDLL(so), "hosttwin")
    return _twin


def gpu_binding():
    from alpha_zero_amd import _lib

    return _lib.load(require_gpu=True)


def backend(kind):
    """kind: 'host' | 'gpu' | 'host:cap2' -> (binding, torch device string)"""
    if kind == "host:cap2":
        return hosttwin_variant("cap2", ["-DAZ_PATH_CAP=2"]), "cpu"
    return (hosttwin_binding(), "cpu") if kind == "host" else (gpu_binding(), "cuda")


# ---------------------------------------------------------------------------------------------------
# environment replay: G games advance in lock-step through azsp_env_step
# ---------------------------------------------------------------------------------------------------
def replay_env_batch(kind, game, n, move_lists, num_to_win=5, num_stack=8):
    """Returns (moves played per game, state digests, observation digests (16 bytes each), final scalars rows int32[G, ENV_COUNT])."""
    binding, dev = backend(kind)
    G = len(move_lists)
    eng = Engine(binding, EngineConfig(game=game, board_size=n, num_games=G, num_parallel=1, num_simulations=2, num_to_win=num_to_win,
                                       num_stack=num_stack, stop_after_move=True), device=dev)
    assert eng.planes == 2 * num_stack + 1
    hs, ho = [hashlib.sha256() for _ in range(G)], [hashlib.sha256() for _ in range(G)]
    played = np.zeros(G, dtype=np.int64)
    alive = np.ones(G, dtype=bool)

    def absorb(out, mask):
        sc = out["scalars"]
        rec = np.concatenate([
            out["board"].reshape(G, -1).view(np.uint8), out["legal"].view(np.uint8),
            np.ascontiguousarray(sc[:, [_abi.ENV_KO, _abi.ENV_CAPS_BLACK, _abi.ENV_CAPS_WHITE, _abi.ENV_STEPS]].astype("<i2")).view(np.uint8).reshape(G, 8),
            np.ascontiguousarray(sc[:, [_abi.ENV_TO_PLAY, _abi.ENV_DONE, _abi.ENV_REWARD]].astype(np.int8)).view(np.uint8)], axis=1)
        assert out["obs"].shape == (G, 2 * num_stack + 1, n, n)
        obs = out["obs"].reshape(G, -1)
        for g in np.flatnonzero(mask):
            hs[g].update(rec[g].tobytes())
            ho[g].update(obs[g].tobytes())

    out = eng.env_step(None, want_obs=True)
    absorb(out, alive)
    final = out["scalars"].copy()
    for t in range(max((len(m) for m in move_lists), default=0)):
        acts = np.array([m[t] if alive[g] and t < len(m) else -2 for g, m in enumerate(move_lists)], dtype=np.int32)
        alive &= acts != -2
        if not alive.any():
            break
        out = eng.env_step(acts, want_obs=True)
        ok = alive & (out["scalars"][:, _abi.ENV_ILLEGAL] == 0)
        absorb(out, ok)
        played += ok
        final[ok] = out["scalars"][ok]
        alive = ok & (out["scalars"][:, _abi.ENV_DONE] == 0)  # stop after the game ended
    eng.close()
    return played, [h.digest()[:16] for h in hs], [h.digest()[:16] for h in ho], final


# ---------------------------------------------------------------------------------------------------
# feature layouts
# ---------------------------------------------------------------------------------------------------
def decode_features(eng):
    """The engine's feature tensor -> int8 planes [rows, 2K+1, N, N], whatever its dtype.  Checks the encoding on the way: only 0 / 1,
    channels 2K+1..31 of the 32-channel layouts zero, the split layout's lo plane never written."""
    rows, n, C = eng.rows, eng.N, eng.planes
    NP = n * n
    f = eng.features
    if eng.features_split:  # AZSP_FEAT_F16_SPLIT: [row][plane: hi, lo][4][n^2][8] f16
        t = f.view(torch.int16).cpu().numpy()[: rows * 2 * 4 * NP * 8].reshape(rows, 2, 4, NP, 8)
        assert not t[:, 1].any(), "lo plane of 0 / 1 observation planes must stay zero"
        x, one = np.ascontiguousarray(t[:, 0].transpose(0, 2, 1, 3)).reshape(rows, NP, 32), 0x3C00
    elif eng.features_tiled:  # AZSP_FEAT_BF16_TILED / _F16_TILED: [tile][4][tb n^2][8]
        tb = max(1, 256 // NP)
        one = 0x3C00 if f.dtype == torch.float16 else 0x3F80
        t = f.view(torch.int16).cpu().numpy().reshape(-1, 4, tb * NP, 8)
        x = np.ascontiguousarray(t.transpose(0, 2, 1, 3)).reshape(-1, 32)[: rows * NP].reshape(rows, NP, 32)
    else:
        x = f.to(torch.float32).cpu().numpy()
        assert x.shape == (rows, C, n, n)
        assert np.all((x == 0) | (x == 1))
        return x.astype(np.int8)
    assert np.all((x == 0) | (x == one)) and not x[:, :, C:].any()
    return np.ascontiguousarray((x[:, :, :C] == one).astype(np.int8).transpose(0, 2, 1)).reshape(rows, C, n, n)


def unsplit_features(flat, rows, n):
    """decode_features for a 17-plane AZSP_FEAT_F16_SPLIT tensor that is not an engine's."""
    return decode_features(SimpleNamespace(features=flat, rows=rows, N=n, planes=17, features_split=True, features_tiled=False))


def split_features(x):
    """[rows, 17, n, n] 0/1 planes -> the AZSP_FEAT_F16_SPLIT tensor (hi plane written, lo plane zero), the inverse of unsplit_features."""
    rows, _, n, _ = x.shape
    NP = n * n
    full = torch.zeros(rows, 2, 4, NP, 8, dtype=torch.float16)
    hi = torch.zeros(rows, NP, 32, dtype=torch.float16)
    hi[:, :, :17] = x.reshape(rows, 17, NP).permute(0, 2, 1).to(torch.float16)
    full[:, 0] = hi.view(rows, NP, 4, 8).permute(0, 2, 1, 3)
    return full.reshape(-1)


def tile_features(x, dtype=torch.bfloat16):
    """[rows, 17, n, n] 0/1 planes -> the AZSP_FEAT_BF16_TILED (or, dtype = float16, _F16_TILED) tensor, what decode_features decodes."""
    rows, _, n, _ = x.shape
    NP = n * n
    tb = max(1, 256 // NP)
    ntiles = (rows + tb - 1) // tb
    full = torch.zeros(ntiles * tb * NP, 32, dtype=dtype)
    full[: rows * NP, :17] = x.reshape(rows, 17, NP).permute(0, 2, 1).reshape(rows * NP, 17).to(dtype)
    return full.view(ntiles, tb * NP, 4, 8).permute(0, 2, 1, 3).contiguous().reshape(-1)


# ---------------------------------------------------------------------------------------------------
# harvested games: the samples of a game row, and what holds for every game
# ---------------------------------------------------------------------------------------------------
def samples_of(row, *arrays):
    """The samples of game row `row` (int32[GR_COUNT]) in each of `arrays` (states / pi / z / moves of the same harvest)."""
    s0 = int(row[_abi.GR_START])
    got = tuple(a[s0:s0 + int(row[_abi.GR_LENGTH])] for a in arrays)
    return got[0] if len(got) == 1 else got


def assert_game_samples(rows, states, z, max_length):
    """Every harvested game: 0 < length <= max_length, the colour plane (the last one) alternates from sample to sample, z is +1 on the
    winner's samples and -1 on the loser's, and 0 everywhere in a game without a winner."""
    for row in rows:
        st, zz = samples_of(row, states, z)
        assert 0 < len(st) == int(row[_abi.GR_LENGTH]) <= max_length
        black = st[:, -1, 0, 0]
        assert np.all(black[1:] != black[:-1])
        winner = int(row[_abi.GR_WINNER])
        if winner != 0:
            wb = 1 if winner == 1 else 0
            assert np.all(zz[black == wb] == 1) and np.all(zz[black != wb] == -1)
        else:
            assert np.all(zz == 0)


def assert_rank_samples_gathered(out, rank, loc):
    """Sample gather (core/gather.py): the game rows of `out` (rank 0's gathered arrays) tagged with `rank` are that rank's own harvest
    `loc`, game by game in START order -- samples byte-identical, rows equal from LENGTH to LAST_PLAYER (START is rebased, SLOT tagged)."""
    games = out["games"]
    mine = games[(games[:, _abi.GR_SLOT] >> _abi.GR_SLOT_RANK_SHIFT) == rank]
    assert len(mine) == len(loc["games"]), (rank, len(mine), len(loc["games"]))
    for row, lrow in zip(mine[np.argsort(mine[:, _abi.GR_START])], loc["games"][np.argsort(loc["games"][:, _abi.GR_START])]):
        for key in ("states", "pi", "z"):
            assert np.array_equal(samples_of(row, out[key]), samples_of(lrow, loc[key]))
        assert np.array_equal(row[_abi.GR_LENGTH:_abi.GR_SLOT], lrow[_abi.GR_LENGTH:_abi.GR_SLOT])


def random_openings(engine, plies, rng):
    """Advance game g of `engine` by plies[g] uniformly random legal board moves (no pass) through the env kernels; returns the
    last env_step output."""
    NP = engine.NP
    out = engine.env_step(None)
    for t in range(int(plies.max())):
        legal = out["legal"][:, :NP].astype(bool)
        r = rng.random(legal.shape) * legal
        acts = np.where((plies > t) & legal.any(axis=1) & (out["scalars"][:, _abi.ENV_DONE] == 0), r.argmax(axis=1), -2).astype(np.int32)
        out = engine.env_step(acts)
    return out


# ---------------------------------------------------------------------------------------------------
# search / actor replay with injected randomness (an MCTS golden file, or the CPU oracle's games)
# ---------------------------------------------------------------------------------------------------
class SearchRun(NamedTuple):
    """What run_injected_search returns: logs[g][k] = dict(pi, child_N, root_q, child_q, move) of game g's k-th logged search, the harvest
    (states, pi, z, games) of every finished game, evaluations per game and ply, the counters, and rows[j][g] = the g-th row of array
    j of `rows_after_move` after every move of slot g (() when nothing was read)."""
    logs: list
    harvest: tuple
    n_evals: np.ndarray
    counters: dict
    rows: tuple


def search_logs(eng, plies):
    """Per game the logged searches (Engine.get_search) of its first plies[g] moves."""
    logs = []
    for gi in range(eng.G):
        per = []
        for k in range(int(plies[gi])):
            pi, cn, q = eng.get_search(gi, k)
            per.append(dict(pi=pi, child_N=cn, root_q=q[_abi.SQ_ROOT_Q], child_q=q[_abi.SQ_CHILD_Q], move=int(q[_abi.SQ_MOVE])))
        logs.append(per)
    return logs


def harvest_all(eng):
    """(states, pi, z, games) of every finished game as host arrays, game rows with START rebased.  The output window may be smaller
    than all finished games: harvest until drained."""
    parts, base = [], 0
    while True:
        states, pi, z, games = eng.harvest()
        if len(games) == 0:
            break
        games = games.copy()
        games[:, _abi.GR_START] += base
        base += len(z)
        parts.append((states.cpu().numpy().copy(), pi.cpu().numpy().copy(), z.cpu().numpy().copy(), games))
    if not parts:
        return (np.zeros((0, eng.planes, eng.N, eng.N), np.int8), np.zeros((0, eng.A), np.float32), np.zeros(0, np.float32),
                np.zeros((0, _abi.GR_COUNT), np.int32))
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(4))


def run_injected_search(kind, noise, unif, eval_batch, plies=None, on_features=None, max_rounds=None, setup=None, on_round=None, inject=True,
                        rows_after_move=None, **engine_kw):
    """The batched actor on noise.shape[0] games with the given randomness injected (noise [G, M, A], unif [G, M, 16]; engine_kw: the
    other EngineConfig fields): select -> eval_batch on the decoded planes of the valid rows -> round, until every game idles.
    setup(eng) runs before the injection and reset_games; inject=False: a seeded engine that draws for itself (noise only gives the
    shape).  on_round(eng, i) runs in front of round i; on_features(round, decoded planes, engine) sees every round; max_rounds: stop
    after that many rounds and return None (feature checks that need no search results).  rows_after_move(eng) -> a tuple of [G, ...]
    arrays, or None to read nothing this round: called at the top of every round, and the rows of the slots whose ply advanced since
    the last one are kept (SearchRun.rows).  plies: the logged searches per game, default all it played.  Returns a SearchRun."""
    binding, dev = backend(kind)
    G, M, A = noise.shape
    eng = Engine(binding, EngineConfig(num_games=G, inject_random=inject, inject_moves=M if inject else 0, stop_at_game_end=True, log_moves=True,
                                       log_capacity=M, **engine_kw), device=dev)
    if setup is not None:
        setup(eng)
    if inject:
        eng.set_injection(noise, unif)
    eng.reset_games()
    eng.counters(reset=True)  # (all zero here unless `setup` ran searches of its own)
    n_evals = np.zeros((G, M), dtype=np.int64)
    kept, seen = (), np.zeros(G, dtype=np.int64)
    eng.select()
    for rounds in range(200000):
        if on_round is not None:
            on_round(eng, rounds)
        valid = eng.valid.cpu().numpy().astype(bool)
        st, _ = eng.status()
        got = rows_after_move(eng) if rows_after_move is not None else None
        if got is not None:
            kept = kept or tuple([[] for _ in range(G)] for _ in got)
            ply = np.minimum(st[:, _abi.STC_PLY], M)
            assert np.all(ply - seen <= 1)  # (a kept sub-tree never holds a whole budget in these shapes: one move per round)
            for g in np.flatnonzero(ply > seen):
                for per, arr in zip(kept, got):
                    per[g].append(arr[g].copy())
            seen = ply.astype(np.int64)
        if not valid.any() and np.all(st[:, _abi.STC_STATUS] == _abi.ST_IDLE):
            break
        feats = decode_features(eng)
        if on_features is not None:
            on_features(rounds, feats, eng)
        if max_rounds is not None and rounds >= max_rounds:
            eng.close()
            return None
        pri = np.zeros((eng.rows, A), dtype=np.float32)
        val = np.zeros(eng.rows, dtype=np.float32)
        rows = np.flatnonzero(valid)
        if len(rows):
            pri[rows], val[rows] = eval_batch(feats[rows], A)
            np.add.at(n_evals, (rows // eng.P, np.minimum(st[rows // eng.P, _abi.STC_PLY], M - 1)), 1)
        eng.priors.copy_(torch.from_numpy(pri))
        eng.values.copy_(torch.from_numpy(val))
        eng.round()
    else:
        raise AssertionError("the games did not finish")
    out = SearchRun(search_logs(eng, np.minimum(st[:, _abi.STC_PLY], M) if plies is None else plies), harvest_all(eng), n_evals, eng.counters(), kept)
    eng.close()
    return out


def run_golden_selfplay(kind, G_gold, eval_batch, feature_dtype=_abi.FEAT_I8, num_stack=None, **kw):
    """run_injected_search on the games of one golden file (golden_mcts.MctsGolden) with its recorded randomness, at the golden's
    num_stack unless given; kw: on_features / max_rounds."""
    g, cfg = G_gold.g, G_gold.cfg
    idxs = [G_gold.moves_of_game(i) for i in range(cfg["games"])]
    M = max(len(ix) for ix in idxs) + 1
    noise, unif = np.zeros((cfg["games"], M, G_gold.A)), np.zeros((cfg["games"], M, 16))
    for gi, ix in enumerate(idxs):
        noise[gi, : len(ix)] = g["noise"][ix]
        unif[gi, : len(ix)] = g["uniforms"][ix]
    return run_injected_search(
        kind, noise, unif, eval_batch, plies=[len(ix) for ix in idxs], game=cfg["game"], board_size=cfg["n"], num_parallel=cfg["parallel"],
        num_simulations=cfg["sims"], c_puct_base=cfg["c_puct_base"], c_puct_init=cfg["c_puct_init"], root_noise=cfg.get("root_noise", True),
        deterministic=cfg.get("deterministic", False), reuse_tree=cfg.get("reuse", True), warm_up_steps=cfg["warm_up_steps"],
        resign_threshold=cfg.get("resign_threshold", -1.0), check_resign_after_steps=cfg.get("check_resign_after_steps", 40),
        force_resign_disabled=1 if cfg.get("resign_disabled", True) else 0, max_plies=cfg.get("max_moves") or 0, feature_dtype=feature_dtype,
        num_stack=G_gold.K if num_stack is None else num_stack, **kw)


# ---------------------------------------------------------------------------------------------------
# engine vs CPU oracle on fresh seeded games (no golden file needed; used by -m gpu tests and smoke())
# ---------------------------------------------------------------------------------------------------
def num_actions(game, n):
    return n * n + (1 if game == "go" else 0)


def make_oracle_env(game, n, max_steps=0, num_to_win=5):
    from oracle.envs import OracleGoEnv, OracleGomokuEnv

    return OracleGoEnv(n, max_steps=max_steps) if game == "go" else OracleGomokuEnv(n, num_to_win=num_to_win)


def empty_positions(n, G):
    """(boards, hist, pos) of BatchSearch.load / Engine.set_states: the empty board with black to move in every one of G slots."""
    boards, hist = np.zeros((G, n, n), np.int8), np.zeros((G, 8, n, n), np.int8)
    pos = np.zeros((G, _abi.PS_COUNT), np.int32)
    pos[:, _abi.PS_TO_PLAY], pos[:, _abi.PS_KO] = 1, -1
    return boards, hist, pos


def small_go9_device_evaluator():
    """(InferenceNet, DeviceEvaluator) of a small seeded 9x9 network on the fp32-class (split-precision) kernels.  (Device only.)"""
    from alpha_zero_amd import _lib
    from alpha_zero_amd.core.evaluate import DeviceEvaluator
    from alpha_zero_amd.core.network import AlphaZeroNet, InferenceNet

    torch.manual_seed(0)
    inf = InferenceNet(AlphaZeroNet((17, 9, 9), 82, 2, 128, 64), dtype=torch.float32, binding=_lib.load()).cuda()
    return inf, DeviceEvaluator(inf)


def shape_table(shapes, **fixed):
    """The two readers of a module's SHAPES table (name -> dict(game, n, sims, G, max_moves, seed[, max_steps, num_to_win])):
    selfplay_args(name, P) = the arguments of oracle_selfplay for that shape, engine_kw(name, P, **more) = the EngineConfig fields of the
    same games (`fixed`: fields every case of the module shares)."""
    def selfplay_args(name, P):
        s = shapes[name]
        return (s["game"], s["n"], s["sims"], P, s["G"], s["seed"], s["max_moves"]), dict(max_steps=s.get("max_steps", 0), num_to_win=s.get("num_to_win", 5))

    def engine_kw(name, P, **more):
        s = shapes[name]
        return dict(game=s["game"], board_size=s["n"], num_parallel=P, num_simulations=s["sims"], max_plies=s["max_moves"], warm_up_steps=4,
                    max_steps=s.get("max_steps", 0), num_to_win=s.get("num_to_win", 5), force_resign_disabled=1, **fixed, **more)

    return selfplay_args, engine_kw


def oracle_selfplay(game, n, sims, P, ngames, seed, max_moves, rule=None, noise=None, unif=None, eval_factory=None, root_noise=True,
                    reuse_tree=True, num_to_win=5, warm_up_steps=4, resign_threshold=-1.0, resign_disabled=True, check_resign_after_steps=40,
                    max_steps=0):
    """Plays `ngames` games with the CPU oracle's actor; returns (noise, uniforms, per game the per-move logs, per game (seq, stats),
    what the rule counted).  noise / unif: the injected rows; None = drawn from PCG64(seed), Dirichlet rows first.  rule: None, or a
    callable that gives a context manager under which the oracle searches by another rule (forced_checks.restated,
    gumbel_checks.restated); it yields a dict whose 'searches' hold one record per finished search, which is merged into that move's
    log (its 'N' as child_N), and whose other entries (event counts, margins) are summed over the games."""
    from oracle import actor, mcts
    from synth_eval import make_eval_func

    rng = np.random.Generator(np.random.PCG64(seed))
    A = num_actions(game, n)
    M = max_moves + 1
    if noise is None:
        noise = rng.dirichlet(np.full(A, 0.03), size=(ngames, M))
    if unif is None:
        unif = rng.random((ngames, M, 16))
    logs, results, counted = [], [], {}
    for gi in range(ngames):
        env = make_oracle_env(game, n, max_steps, num_to_win)
        per = []

        def on_move(k, env_, move, pi, rq, cq, root):
            cn = root.N[root.parent[root.root]].copy() if root is not None else None
            per.append(dict(move=int(move), pi=np.asarray(pi, dtype=np.float64), root_q=float(rq), child_q=float(cq), child_N=cn))

        with (rule() if rule is not None else contextlib.nullcontext(dict(searches=[]))) as rec:
            seq, stats = actor.play_one_game(
                env, (eval_factory or make_eval_func)(A), num_simulations=sims, num_parallel=P, warm_up_steps=warm_up_steps,
                check_resign_after_steps=check_resign_after_steps, resign_threshold=resign_threshold, resign_disabled=resign_disabled,
                root_noise=root_noise, reuse_tree=reuse_tree, rand_for_move=lambda k: mcts.InjectedRand(noise[gi, k], unif[gi, k]),
                on_move=on_move, max_moves=max_moves)
        assert rule is None or len(rec["searches"]) >= len(per)
        for move, s in zip(per, rec["searches"]):
            assert move["move"] == s.get("move", move["move"])
            move.update(s, child_N=s["N"])
        for key, v in rec.items():
            if key != "searches":
                counted[key] = counted[key] + v if key in counted else v
        logs.append(per)
        results.append((seq, stats))
    return noise, unif, logs, results, counted


def compare_engine_with_oracle(kind, game, n, sims, P, ngames, seed, max_moves, **kw):
    """Bit-exact comparison of the engine with the oracle on seeded games; returns the engine counters."""
    from alpha_zero_amd.core.pipeline import game_stats_from_row
    from synth_eval import eval_batch

    noise, unif, ologs, ores, _ = oracle_selfplay(game, n, sims, P, ngames, seed, max_moves, **kw)
    elogs, (states, pis, zs, games), _, cnt, _ = run_injected_search(
        kind, noise, unif, eval_batch, game=game, board_size=n, num_parallel=P, num_simulations=sims, max_plies=max_moves,
        warm_up_steps=kw.get("warm_up_steps", 4), resign_threshold=kw.get("resign_threshold", -1.0),
        check_resign_after_steps=kw.get("check_resign_after_steps", 40), force_resign_disabled=1 if kw.get("resign_disabled", True) else 0,
        max_steps=kw.get("max_steps", 0))
    by_slot = {int(r[_abi.GR_SLOT]): r for r in games}
    for gi in range(ngames):
        assert len(elogs[gi]) == len(ologs[gi]), (gi, len(elogs[gi]), len(ologs[gi]))
        for k, (e, o) in enumerate(zip(elogs[gi], ologs[gi])):
            where = (game, n, gi, k)
            assert e["move"] == o["move"], where
            if o["child_N"] is not None:
                assert np.array_equal(e["child_N"], o["child_N"]), where
            assert e["root_q"] == o["root_q"] and e["child_q"] == o["child_q"], where
            if game == "go":
                assert np.array_equal(e["pi"], o["pi"]), where
            else:
                assert np.abs(e["pi"] - o["pi"]).max() <= 1e-6, where
        seq, stats = ores[gi]
        if seq is None:
            assert gi not in by_slot
            continue
        row = by_slot[gi]
        gst, gz = samples_of(row, states, zs)
        assert len(gst) == len(seq)
        assert np.array_equal(gst, np.stack([t.state for t in seq]))
        assert np.array_equal(gz, np.array([t.value for t in seq], dtype=np.float32))
        est = game_stats_from_row(row, game=game, komi=7.5, resign_threshold=kw.get("resign_threshold", -1.0))
        assert est == stats, (est, stats)
    return cnt
