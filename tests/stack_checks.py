"""Drivers and assertions of the num_stack tests (observation history depth K = 1..8, 2K+1 planes), shared by the host twin
(tests/test_num_stack_host.py) and the GPU (tests/test_num_stack_gpu.py).  The goldens (tests/golden/stack_*.npz) come from the
reference at K < 8 (tools/gen_golden_stack.py)."""
import hashlib
import json
import os

import numpy as np
import torch

import engine_util as eu
from alpha_zero_amd import _abi
from alpha_zero_amd.core.engine import Engine, EngineConfig
from alpha_zero_amd.core.pipeline import game_stats_from_row
from synth_eval import eval_batch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PLAYOUTS = [("go", 9, 1), ("go", 9, 4), ("go", 19, 2), ("gomoku", 13, 1), ("gomoku", 13, 4)]
MCTS = ["go9_p8_s200_k4", "go5_p4_s48_k2", "gomoku13_p8_s200_k1"]
FEATS = {"i8": _abi.FEAT_I8, "f32": _abi.FEAT_F32, "bf16": _abi.FEAT_BF16_TILED, "f16": _abi.FEAT_F16_TILED, "f16_split": _abi.FEAT_F16_SPLIT}


# ---------------------------------------------------------------------------------------------------
# feature layouts with 2K+1 planes
# ---------------------------------------------------------------------------------------------------
def decode_features(eng):
    """The engine's feature tensor -> int8 planes [rows, 2K+1, N, N], whatever its dtype.  Checks the encoding of the 32-channel
    layouts on the way: only 0 / 1, channels 2K+1..31 zero, the split layout's lo plane never written."""
    rows, n, C = eng.rows, eng.N, eng.planes
    NP = n * n
    f = eng.features
    if eng.features_split:
        t = f.view(torch.int16).cpu().numpy()[: rows * 2 * 4 * NP * 8].reshape(rows, 2, 4, NP, 8)
        assert not t[:, 1].any(), "lo plane of 0 / 1 observation planes must stay zero"
        x, one = np.ascontiguousarray(t[:, 0].transpose(0, 2, 1, 3)).reshape(rows, NP, 32), 0x3C00
    elif eng.features_tiled:
        tb = max(1, 256 // NP)
        one = 0x3C00 if f.dtype == torch.float16 else 0x3F80
        t = f.view(torch.int16).cpu().numpy().reshape(-1, 4, tb * NP, 8)
        x = np.ascontiguousarray(t.transpose(0, 2, 1, 3)).reshape(-1, 32)[: rows * NP].reshape(rows, NP, 32)
    else:
        x = f.cpu().numpy()
        assert x.shape == (rows, C, n, n)
        assert np.all((x == 0) | (x == 1))
        return x.astype(np.int8)
    assert np.all((x == 0) | (x == one)) and not x[:, :, C:].any()
    return np.ascontiguousarray((x[:, :, :C] == one).astype(np.int8).transpose(0, 2, 1)).reshape(rows, C, n, n)


# ---------------------------------------------------------------------------------------------------
# environment replay (azsp_env_step) vs the reference's playout digests
# ---------------------------------------------------------------------------------------------------
def replay_digests(kind, game, n, num_stack, move_lists):
    binding, dev = eu.backend(kind)
    G = len(move_lists)
    eng = Engine(binding, EngineConfig(game=game, board_size=n, num_games=G, num_parallel=1, num_simulations=2, num_stack=num_stack,
                                       stop_after_move=True), device=dev)
    assert eng.planes == 2 * num_stack + 1
    hs, ho = [hashlib.sha256() for _ in range(G)], [hashlib.sha256() for _ in range(G)]
    played = np.zeros(G, dtype=np.int64)
    alive = np.ones(G, dtype=bool)

    def absorb(out, mask):
        sc = out["scalars"]
        rec = np.concatenate([
            out["board"].reshape(G, -1).view(np.uint8), out["legal"].view(np.uint8),
            np.ascontiguousarray(sc[:, [0, 1, 2, 3]].astype("<i2")).view(np.uint8).reshape(G, 8),
            np.ascontiguousarray(sc[:, [4, 5, 6]].astype(np.int8)).view(np.uint8)], axis=1)
        assert out["obs"].shape == (G, 2 * num_stack + 1, n, n)
        obs = out["obs"].reshape(G, -1)
        for g in np.flatnonzero(mask):
            hs[g].update(rec[g].tobytes())
            ho[g].update(obs[g].tobytes())

    eng.reset_games()
    absorb(eng.env_step(None, want_obs=True), alive)
    for t in range(max(len(m) for m in move_lists)):
        acts = np.array([m[t] if alive[g] and t < len(m) else -2 for g, m in enumerate(move_lists)], dtype=np.int32)
        alive &= acts != -2
        if not alive.any():
            break
        out = eng.env_step(acts, want_obs=True)
        ok = alive & (out["scalars"][:, 10] == 0)
        absorb(out, ok)
        played += ok
        alive = ok & (out["scalars"][:, 5] == 0)
    eng.close()
    return played, [h.digest()[:16] for h in hs], [h.digest()[:16] for h in ho]


def check_playouts(kind, game, n, k):
    g = np.load(os.path.join(GOLDEN, f"stack_{game}{n}_k{k}_random.npz"))
    off, mv = g["offsets"], g["moves"]
    lists = [mv[off[i]:off[i + 1]].astype(np.int32) for i in range(len(off) - 1)]
    played, ds, do = replay_digests(kind, game, n, k, lists)
    bad = [i for i in range(len(lists)) if played[i] != len(lists[i]) or ds[i] != g["state_digest"][i].tobytes()
           or do[i] != g["obs_digest"][i].tobytes()]
    assert len(lists) > 0 and not bad, bad[:5]


# ---------------------------------------------------------------------------------------------------
# batched actor with the recorded randomness injected vs the reference's search / actor goldens
# ---------------------------------------------------------------------------------------------------
class StackGolden:
    def __init__(self, name):
        self.g = np.load(os.path.join(GOLDEN, f"stack_mcts_{name}.npz"))
        self.cfg = json.loads(str(self.g["config"]))
        self.A, self.K = self.cfg["num_actions"], self.cfg["num_stack"]

    def moves_of_game(self, gi):
        return np.flatnonzero(self.g["game"] == gi)

    def finished(self, gi):
        return bool(int(self.g[f"g{gi}_finished"]))

    def samples(self, gi):
        n, C = self.cfg["n"], 2 * self.K + 1
        st = np.unpackbits(self.g[f"g{gi}_states"], axis=1)[:, : C * n * n].reshape(-1, C, n, n).astype(np.int8)
        return st, self.g[f"g{gi}_pis"], self.g[f"g{gi}_zs"], json.loads(str(self.g[f"g{gi}_stats"]))


def run_selfplay(kind, G_gold, feature_dtype=_abi.FEAT_I8, on_features=None, num_stack=None, max_rounds=None):
    """The golden's games on one engine (num_stack of the golden unless given); on_features(round, decoded planes, engine) per round.
    max_rounds: stop after that many rounds and return None (feature checks that need no search results)."""
    g, cfg = G_gold.g, G_gold.cfg
    binding, dev = eu.backend(kind)
    ngames, A = cfg["games"], G_gold.A
    idxs = [G_gold.moves_of_game(i) for i in range(ngames)]
    M = max(len(ix) for ix in idxs) + 1
    noise, unif = np.zeros((ngames, M, A)), np.zeros((ngames, M, 16))
    for gi, ix in enumerate(idxs):
        noise[gi, : len(ix)] = g["noise"][ix]
        unif[gi, : len(ix)] = g["uniforms"][ix]
    ec = EngineConfig(
        game=cfg["game"], board_size=cfg["n"], num_games=ngames, num_parallel=cfg["parallel"], num_simulations=cfg["sims"],
        c_puct_base=cfg["c_puct_base"], c_puct_init=cfg["c_puct_init"], root_noise=cfg.get("root_noise", True),
        deterministic=cfg.get("deterministic", False), reuse_tree=cfg.get("reuse", True), warm_up_steps=cfg["warm_up_steps"],
        resign_threshold=cfg.get("resign_threshold", -1.0), check_resign_after_steps=cfg.get("check_resign_after_steps", 40),
        force_resign_disabled=1 if cfg.get("resign_disabled", True) else 0, inject_random=True, inject_moves=M,
        max_plies=cfg.get("max_moves") or 0, stop_at_game_end=True, feature_dtype=feature_dtype, log_moves=True, log_capacity=M,
        num_stack=G_gold.K if num_stack is None else num_stack)
    eng = Engine(binding, ec, device=dev)
    eng.set_injection(noise, unif)
    eng.reset_games()
    n_evals = np.zeros((ngames, M), dtype=np.int64)
    rounds = 0
    eng.select()
    while True:
        valid = eng.valid.cpu().numpy().astype(bool)
        st, _ = eng.status()
        if not valid.any() and np.all(st[:, 0] == _abi.ST_IDLE):
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
            for r in rows:
                n_evals[r // eng.P, min(st[r // eng.P, 1], M - 1)] += 1
        eng.priors.copy_(torch.from_numpy(pri))
        eng.values.copy_(torch.from_numpy(val))
        eng.round()
        rounds += 1
        assert rounds < 200000
    logs = []
    for gi, ix in enumerate(idxs):
        per = []
        for k in range(len(ix)):
            pi, cn, q = eng.get_search(gi, k)
            per.append(dict(pi=pi, child_N=cn, root_q=q[0], child_q=q[1], move=int(q[3])))
        logs.append(per)
    parts, base = [], 0
    while True:
        states, pi, z, games = eng.harvest()
        if len(games) == 0:
            break
        games = games.copy()
        games[:, 0] += base
        base += len(z)
        parts.append((states.cpu().numpy().copy(), pi.cpu().numpy().copy(), z.cpu().numpy().copy(), games))
    C = eng.planes
    hv = (tuple(np.concatenate([p[i] for p in parts]) for i in range(4)) if parts else
          (np.zeros((0, C, eng.N, eng.N), np.int8), np.zeros((0, A), np.float32), np.zeros(0, np.float32), np.zeros((0, 16), np.int32)))
    eng.close()
    return logs, hv, n_evals


def check_mcts(kind, name, feature_dtype=_abi.FEAT_I8):
    """Bit-exact like tests/parity_checks.py check_mcts_golden: visit counts, moves, root_Q / best_child_Q, evaluation counts, Go pi;
    the (state, pi, z) samples of finished games with 2K+1 planes and their stats.  Gomoku pi (float32 in the reference) <= 1e-6."""
    G = StackGolden(name)
    g, cfg = G.g, G.cfg
    logs, (states, pis, zs, games), n_evals = run_selfplay(kind, G, feature_dtype)
    for gi in range(cfg["games"]):
        for k, i in enumerate(G.moves_of_game(gi)):
            L, where = logs[gi][k], (name, gi, k)
            assert np.array_equal(L["child_N"], g["child_N"][i]), where
            assert L["move"] == g["move"][i], where
            assert L["root_q"] == g["root_q"][i] and L["child_q"] == g["child_q"][i], where
            if cfg["game"] == "go":
                assert np.array_equal(L["pi"], g["pi"][i]), where
            else:
                assert np.abs(L["pi"] - g["pi"][i]).max() <= 1e-6, where
            assert n_evals[gi, k] == g["n_evals"][i], where
    assert states.shape[1] == 2 * G.K + 1
    by_slot = {int(row[15]): row for row in games}
    finished = 0
    for gi in range(cfg["games"]):
        if not G.finished(gi):
            assert gi not in by_slot
            continue
        finished += 1
        st, gp, gz, gstats = G.samples(gi)
        row = by_slot[gi]
        s0, ln = int(row[0]), int(row[1])
        assert ln == len(st)
        assert np.array_equal(states[s0:s0 + ln], st)
        assert np.array_equal(zs[s0:s0 + ln], gz.astype(np.float32))
        if cfg["game"] == "go":
            assert np.array_equal(pis[s0:s0 + ln], gp.astype(np.float32))
        else:
            assert np.abs(pis[s0:s0 + ln] - gp).max() <= 1e-6
        stats = game_stats_from_row(row, game=cfg["game"], komi=7.5, resign_threshold=cfg.get("resign_threshold", -1.0))
        assert json.loads(json.dumps(stats)) == gstats, (stats, gstats)
    return finished
