"""Python host of the batched self-play engine: thin object wrapper over the C ABI (include/azsp.h).

All per-game state (trees, positions, samples) lives in HBM inside the engine; this class only owns
the evaluator-facing tensors (features / valid / priors / values) and passes raw device pointers.
Nothing here computes on the CPU except the tiny pb_c / sqrt lookup tables, which are evaluated with
the very expressions of the reference (mcts_v2.py:99-102) so their rounding is identical.
"""
import ctypes as C
import math
from dataclasses import dataclass

import numpy as np
import torch

from .. import _abi
from .._abi import AzspConfig, AzspGeometry, Binding

_FEAT_TORCH = {_abi.FEAT_I8: torch.int8, _abi.FEAT_F32: torch.float32, _abi.FEAT_BF16: torch.bfloat16, _abi.FEAT_F16: torch.float16}


@dataclass
class EngineConfig:
    game: str = "go"                 # "go" | "gomoku"
    board_size: int = 9
    num_games: int = 1
    num_parallel: int = 8
    num_simulations: int = 200
    c_puct_base: float = 19652.0
    c_puct_init: float = 1.25
    root_noise: bool = True
    deterministic: bool = False
    reuse_tree: bool = True
    warm_up_steps: int = 16
    komi: float = 7.5
    max_steps: int = 0
    num_to_win: int = 5
    num_stack: int = 8               # history boards per observation (base.py:228-266): 2 * num_stack + 1 planes, 1..8
    resign_threshold: float = -1.0
    check_resign_after_steps: int = 40
    disable_resign_ratio: float = 0.1
    force_resign_disabled: int = -1
    dirichlet_eps: float = 0.25
    dirichlet_alpha: float = 0.03
    inject_random: bool = False
    inject_moves: int = 0
    stop_after_move: bool = False
    max_plies: int = 0
    stop_at_game_end: bool = False
    feature_dtype: int = _abi.FEAT_F32
    log_moves: bool = False
    log_capacity: int = 0
    max_nodes: int = 0
    training_steps: int = 0
    seed: int = 1
    rank: int = 0
    device_index: int = 0
    leaf_symmetry: object = None     # the opt-in search rules, as SearchOptions.of takes them: None | "random" | 0..7,
    forced_playouts: object = None   # None | k >= 0,
    gumbel: object = None            # None | m | (m, c_visit, c_scale),
    fpu_reduction: object = None     # None | r | (r_tree, r_root)
    aux_targets: bool = False        # auxiliary training targets per sample (Engine.set_aux_targets; harvest(with_aux=True))
    policy_surprise: object = None   # policy surprise weighting (Engine.set_policy_surprise; harvest(with_surprise=True)): None | frac | (frac, include_fast)
    visit_reduction: object = None   # decided-game visit reduction (Engine.set_visit_reduction; harvest(with_base=True)): None | (threshold, lookback, min_simulations, min_weight)


def leaf_symmetry_mode(mode):
    """The azsp_set_leaf_symmetry argument of a `leaf_symmetry` value: None = off, "random" = a fresh op per feature row, an integer
    0..7 = that dihedral op for every row.  Anything else raises ValueError naming these."""
    if mode is None:
        return _abi.SYM_OFF
    if isinstance(mode, str) and mode == "random":
        return _abi.SYM_RANDOM
    if not isinstance(mode, (bool, str)) and isinstance(mode, (int, np.integer)) and 0 <= int(mode) <= 7:
        return int(mode)
    raise ValueError(f'leaf_symmetry must be None (off), "random" or an integer op 0..7, got {mode!r}')


def forced_playouts_k(k):
    """The azsp_set_forced_playouts factor of a `forced_playouts` value: None = off (0.0), else a finite number k >= 0 (KataGo uses 2).
    Anything else raises ValueError naming these."""
    if k is None:
        return 0.0
    if not isinstance(k, (bool, str)) and isinstance(k, (int, float, np.integer, np.floating)) and math.isfinite(float(k)) and float(k) >= 0.0:
        return float(k)
    raise ValueError(f"forced_playouts must be None (off) or a finite number k >= 0, got {k!r}")


def gumbel_params(gumbel):
    """The azsp_set_gumbel arguments (m, c_visit, c_scale) of a `gumbel` value: None = off (m = 0), an integer m >= 0 (c_visit = 50,
    c_scale = 1.0, the paper's), or (m, c_visit, c_scale) with finite c_visit, c_scale >= 0.  Anything else raises ValueError naming these."""
    is_int = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, bool)  # noqa: E731
    is_num = lambda v: (not isinstance(v, (bool, str)) and isinstance(v, (int, float, np.integer, np.floating))  # noqa: E731
                        and math.isfinite(float(v)) and float(v) >= 0.0)
    if gumbel is None:
        return 0, 50.0, 1.0
    if is_int(gumbel) and 0 <= int(gumbel) < 2 ** 31:
        return int(gumbel), 50.0, 1.0
    if isinstance(gumbel, (tuple, list)) and len(gumbel) == 3 and is_int(gumbel[0]) and 0 <= int(gumbel[0]) < 2 ** 31 and is_num(gumbel[1]) \
            and is_num(gumbel[2]):
        return int(gumbel[0]), float(gumbel[1]), float(gumbel[2])
    raise ValueError(f"gumbel must be None (off), an integer m >= 0 or (m, c_visit, c_scale) with finite c_visit, c_scale >= 0, got {gumbel!r}")


def fpu_params(value):
    """The azsp_set_fpu arguments (on, r_tree, r_root) of an `fpu_reduction` value: None = off, a finite number r >= 0 = that reduction
    at every node, or (r_tree, r_root) = below the root and at it (KataGo: (0.2, 0.1)).  0 is on: an unvisited child is then worth its
    parent's value.  Anything else raises ValueError naming these."""
    is_num = lambda v: (not isinstance(v, (bool, str, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating))  # noqa: E731
                        and math.isfinite(float(v)) and float(v) >= 0.0)
    if value is None:
        return 0, 0.0, 0.0
    if is_num(value):
        return 1, float(value), float(value)
    if isinstance(value, (tuple, list)) and len(value) == 2 and is_num(value[0]) and is_num(value[1]):
        return 1, float(value[0]), float(value[1])
    raise ValueError(f"fpu_reduction must be None (off), a finite number r >= 0 or (r_tree, r_root) of two such numbers, got {value!r}")


def policy_surprise_params(value):
    """The azsp_set_policy_surprise arguments (on, frac, include_fast) of a `policy_surprise` value: None = off, a number frac in [0, 1]
    = on with that share of every game's weight handed out by surprise (fast moves of a playout cap take no part), or
    (frac, include_fast).  Anything else raises ValueError naming these."""
    is_frac = lambda v: (not isinstance(v, (bool, str)) and isinstance(v, (int, float, np.integer, np.floating))  # noqa: E731
                         and 0.0 <= float(v) <= 1.0)
    if value is None:
        return 0, 0.0, 0
    if is_frac(value):
        return 1, float(value), 0
    if isinstance(value, (tuple, list)) and len(value) == 2 and is_frac(value[0]) and isinstance(value[1], (bool, np.bool_)):
        return 1, float(value[0]), int(bool(value[1]))
    raise ValueError(f"policy_surprise must be None (off), a number frac in [0, 1] or (frac, include_fast: bool), got {value!r}")


def visit_reduction_params(value, num_simulations=None):
    """The azsp_set_visit_reduction arguments (lookback, threshold, min_simulations, min_weight) of a `visit_reduction` value: None = off,
    or (threshold in [0, 1), lookback in 1..8, min_simulations in 1..num_simulations, min_weight in [0, 1]).  Anything else raises
    ValueError naming these."""
    num = lambda v: not isinstance(v, (bool, str)) and isinstance(v, (int, float, np.integer, np.floating))  # noqa: E731
    whole = lambda v: not isinstance(v, bool) and isinstance(v, (int, np.integer))  # noqa: E731
    if value is None:
        return 0, 0.0, 1, 1.0
    if isinstance(value, (tuple, list)) and len(value) == 4:
        t, look, sims, w = value
        if (num(t) and 0.0 <= float(t) < 1.0 and whole(look) and 1 <= int(look) <= 8 and whole(sims) and int(sims) >= 1
                and (num_simulations is None or int(sims) <= num_simulations) and num(w) and 0.0 <= float(w) <= 1.0):
            return int(look), float(t), int(sims), float(w)
    raise ValueError("visit_reduction must be None (off) or (threshold in [0, 1), lookback in 1..8, min_simulations in 1..num_simulations, "
                     f"min_weight in [0, 1]), got {value!r}")


EXCLUSIVE = "gumbel and forced_playouts cannot be on together: both decide what the root selects"


@dataclass(frozen=True)
class SearchOptions:
    """The opt-in search rules of one engine, validated: what EngineConfig, dropin_engine, BatchSearch, SelfPlayActor and
    run_selfplay_actor_loop take as `leaf_symmetry`, `forced_playouts`, `prune_policy_target`, `gumbel`, `playout_cap` and `fpu_reduction`."""
    leaf_symmetry: object = None         # as given: None | "random" | 0..7
    forced_k: float = 0.0                # 0.0 = off
    prune_policy_target: bool = True
    gumbel: tuple = (0, 50.0, 1.0)       # (m, c_visit, c_scale), m = 0 = off
    playout_cap: object = None           # None | (fast_simulations, full_prob)
    fpu: tuple = (0, 0.0, 0.0)           # (on, r_tree, r_root)

    @classmethod
    def of(cls, leaf_symmetry=None, forced_playouts=None, prune_policy_target=True, gumbel=None, playout_cap=None, num_simulations=None,
           fpu_reduction=None):
        """The one place these values are checked (ValueError naming the allowed ones); the reference search has none of the rules and
        all are off by default.
        leaf_symmetry: None, "random" or an op 0..7 (Engine.set_leaf_symmetry): every leaf position is evaluated under that board
        symmetry -- "random": one drawn per feature row -- and its priors are mapped back before the node is expanded; the evaluator sees
        nothing but a different board, and pi, child_N, Q and harvested samples stay in the true orientation.
        forced_playouts: None or a finite k >= 0 (Engine.set_forced_playouts; KataGo's, k = 2 there): in every search that is no fast
        move of the playout cap, a root child in play gets at least sqrt(k P(c) sum N) visits.  The move is chosen from the unpruned
        policy; prune_policy_target: the recorded pi rows (Engine.target_policies, the harvest) leave out the forced visits the search
        did not want, False records the plain policy of the forced search.
        gumbel: None, m or (m, c_visit, c_scale) (Engine.set_gumbel; Gumbel AlphaZero, Danihelka et al. 2022): every search that is no
        fast move samples m root actions with Gumbel noise instead of adding Dirichlet noise, spends its simulations on them by
        sequential halving, ends with the move a* (Engine.gumbel_moves; the actor plays it whatever warm-up and `deterministic` say)
        and records softmax(logits + sigma(completed Q)) as the pi row.  Not together with forced_playouts.
        playout_cap: None or (fast_simulations, full_prob) (Engine.set_playout_cap; the batched actor only): a move is a full search
        (the slot's budget, root noise) with probability full_prob, else a fast one of fast_simulations (1..num_simulations, the upper
        end checked where `num_simulations` is given) without noise that only moves the game on.
        fpu_reduction: None, r or (r_tree, r_root), finite and >= 0 (Engine.set_fpu_reduction; first-play urgency reduction as in Leela
        Zero and KataGo, (0.2, 0.1) there): an unvisited child is scored with its parent's own value minus r sqrt(prior mass of the
        visited children) in place of a draw.  Every search follows it, fast moves too; under gumbel it holds below the root."""
        leaf_symmetry_mode(leaf_symmetry)
        k, g, fpu = forced_playouts_k(forced_playouts), gumbel_params(gumbel), fpu_params(fpu_reduction)
        if g[0] > 0 and k > 0.0:
            raise ValueError(EXCLUSIVE)
        if playout_cap is not None:
            fast, prob = playout_cap
            top = float("inf") if num_simulations is None else num_simulations
            if isinstance(fast, bool) or not isinstance(fast, (int, np.integer)) or not 1 <= fast <= top or not 0.0 <= float(prob) <= 1.0:
                raise ValueError(f"playout_cap must be (fast_simulations in 1..{num_simulations}, full_prob in [0, 1]), got {playout_cap!r}")
            playout_cap = (int(fast), float(prob))
        return cls(leaf_symmetry, k, bool(prune_policy_target), g, playout_cap, fpu)


MAX_NUM_STACK = 8  # the engine's history ring holds 8 boards (include/azsp.h AzspConfig.num_stack)


def check_num_stack(num_stack):
    """num_stack (history boards per observation) must be an integer in 1..MAX_NUM_STACK; raises ValueError naming the limit."""
    if isinstance(num_stack, bool) or not isinstance(num_stack, (int, np.integer)) or not 1 <= int(num_stack) <= MAX_NUM_STACK:
        raise ValueError(f"num_stack must be an integer in 1..{MAX_NUM_STACK} (the engine keeps {MAX_NUM_STACK} history boards), got {num_stack!r}")
    return int(num_stack)


def pbc_tables(c_puct_base, c_puct_init, n):
    """pb_c(N) as the reference evaluates it (mcts_v2.py:101): N is an np.float32 for interior nodes and
    re-used roots, a Python float for a freshly created root; sqrt(N) is a Python double that NumPy
    narrows to float32 when it divides the float32 row (mcts_v2.py:102)."""
    t_np = np.array([math.log((1 + np.float32(i) + c_puct_base) / c_puct_base) + c_puct_init for i in range(n)], dtype=np.float64)
    t_py = np.array([math.log((1 + float(i) + c_puct_base) / c_puct_base) + c_puct_init for i in range(n)], dtype=np.float64)
    sq = np.array([np.float32(math.sqrt(np.float32(i))) for i in range(n)], dtype=np.float32)
    return t_np, t_py, sq


class Engine:
    """One engine = G concurrent games on one device.  `binding` comes from alpha_zero_amd._lib.load()."""

    def __init__(self, binding: Binding, cfg: EngineConfig, device="cuda", prune_policy_target=True, playout_cap=None):
        """cfg.leaf_symmetry / .forced_playouts / .gumbel / .fpu_reduction, prune_policy_target and playout_cap: SearchOptions.of."""
        opt = SearchOptions.of(cfg.leaf_symmetry, cfg.forced_playouts, prune_policy_target, cfg.gumbel, playout_cap, cfg.num_simulations,
                               cfg.fpu_reduction)
        self.b, self.cfg, self.device = binding, cfg, torch.device(device)
        self.on_launch = None
        check_num_stack(cfg.num_stack)
        c = AzspConfig()
        c.game = _abi.GAME_GO if cfg.game == "go" else _abi.GAME_GOMOKU
        c.board_size, c.num_games, c.num_parallel, c.num_simulations = cfg.board_size, cfg.num_games, cfg.num_parallel, cfg.num_simulations
        c.max_nodes, c.root_noise, c.deterministic, c.reuse_tree = cfg.max_nodes, int(cfg.root_noise), int(cfg.deterministic), int(cfg.reuse_tree)
        c.warm_up_steps = cfg.warm_up_steps
        c.has_resign = 1 if cfg.game == "go" else 0
        c.check_resign_after_steps, c.force_resign_disabled = cfg.check_resign_after_steps, cfg.force_resign_disabled
        c.inject_random, c.inject_moves = int(cfg.inject_random), cfg.inject_moves
        c.stop_after_move, c.max_plies, c.stop_at_game_end = int(cfg.stop_after_move), cfg.max_plies, int(cfg.stop_at_game_end)
        c.feature_dtype, c.log_moves, c.log_capacity = cfg.feature_dtype, int(cfg.log_moves), cfg.log_capacity
        c.max_steps, c.num_to_win, c.training_steps, c.rank = cfg.max_steps, cfg.num_to_win, cfg.training_steps, cfg.rank
        c.device = cfg.device_index
        c.c_puct_base, c.c_puct_init, c.disable_resign_ratio = cfg.c_puct_base, cfg.c_puct_init, cfg.disable_resign_ratio
        c.dirichlet_eps, c.dirichlet_alpha, c.resign_threshold, c.komi = cfg.dirichlet_eps, cfg.dirichlet_alpha, cfg.resign_threshold, cfg.komi
        c.seed, c.num_stack = cfg.seed, cfg.num_stack
        self.h = C.c_void_p()
        self.b.check(self.b.dll.azsp_create(C.byref(c), C.byref(self.h)), None, "azsp_create")
        g = AzspGeometry()
        self._ck(self.b.dll.azsp_geometry(self.h, C.byref(g)), "azsp_geometry")
        self.geo = g
        self.A, self.NP, self.N, self.G, self.P = g.num_actions, g.num_points, cfg.board_size, cfg.num_games, cfg.num_parallel
        self.rows = g.batch_rows
        self.planes = g.planes  # 2 * num_stack + 1 observation planes per row
        t_np, t_py, sq = pbc_tables(cfg.c_puct_base, cfg.c_puct_init, g.table_len)
        self._ck(self.b.dll.azsp_set_tables(self.h, t_np.ctypes.data, t_py.ctypes.data, sq.ctypes.data, g.table_len), "azsp_set_tables")
        # evaluator-facing tensors (caller-visible; the engine reads / writes them in place)
        self.features_tiled = cfg.feature_dtype in (_abi.FEAT_BF16_TILED, _abi.FEAT_F16_TILED)
        self.features_split = cfg.feature_dtype == _abi.FEAT_F16_SPLIT
        if self.features_split:  # the fp32-class stem's input (AZSP_FEAT_F16_SPLIT): [row][hi, lo][4][N*N][8] f16; only hi planes are ever written
            self.features = torch.zeros((self.b.dll.azsp_split_bytes(self.rows, self.N, 32) // 2,), dtype=torch.float16, device=self.device)
        elif self.features_tiled:  # the evaluator's tiled layout (include/azsp.h: AZSP_FEAT_BF16_TILED / _F16_TILED), flat and zero-initialised
            n = self.b.dll.azsp_tiled_bytes(self.rows, self.N, 32) // 2
            self.features = torch.zeros((n,), dtype=torch.float16 if cfg.feature_dtype == _abi.FEAT_F16_TILED else torch.bfloat16, device=self.device)
        else:
            self.features = torch.zeros((self.rows, self.planes, self.N, self.N), dtype=_FEAT_TORCH[cfg.feature_dtype], device=self.device)
        self.valid = torch.zeros((self.rows,), dtype=torch.uint8, device=self.device)
        self.priors = torch.zeros((self.rows, self.A), dtype=torch.float32, device=self.device)
        self.values = torch.zeros((self.rows,), dtype=torch.float32, device=self.device)
        self._actions = torch.zeros((self.G,), dtype=torch.int32, device=self.device)
        self._harvest_bufs = None
        self._forced_k, self._gumbel_m = 0.0, 0  # what is on now: the two rules exclude each other
        # each has been on at least once, so its rows exist: the target rows (target_policies); the n0 rows too (gumbel_moves)
        self.forced_playouts = self.gumbel = False
        if opt.leaf_symmetry is not None:
            self.set_leaf_symmetry(opt.leaf_symmetry)  # before the first select: the first root evaluation is transformed too
        if opt.forced_k > 0.0:
            self.set_forced_playouts(opt.forced_k, opt.prune_policy_target)
        if opt.gumbel[0] > 0:
            self.set_gumbel(opt.gumbel)
        if opt.playout_cap is not None:
            self.set_playout_cap(*opt.playout_cap)  # before the first root: the first move of every game draws its class too
        self.fpu_reduction = None  # what is on now: None or (r_tree, r_root)
        if opt.fpu[0]:
            self.set_fpu_reduction(opt.fpu[1:])  # before the first select
        self.aux_targets = False  # has been on at least once, so the staging rows exist (harvest(with_aux=True))
        self._harvest_aux_bufs = None
        if cfg.aux_targets:
            self.set_aux_targets(True)  # before the first move is recorded
        self.policy_surprise = False  # has been on at least once, so the staging row exists (harvest(with_surprise=True))
        self._harvest_surprise_bufs = None
        if cfg.policy_surprise is not None:
            self.set_policy_surprise(cfg.policy_surprise)  # before the first move is recorded
        self.visit_reduction = False  # has been on at least once, so the staging row exists (harvest(with_base=True))
        self._harvest_base_bufs = None
        if cfg.visit_reduction is not None:
            self.set_visit_reduction(cfg.visit_reduction)  # before the first move starts

    # -- plumbing ---------------------------------------------------------------------------------
    def _ck(self, rc, what):
        self.b.check(rc, self.h, what)

    def _stream(self):
        if self.device.type == "cuda":
            cur = torch.cuda.current_stream(self.device)
            if self.on_launch is not None:  # experiment hook (tools/overlap_actor.py joins its two half-batch streams here); never set by the product
                self.on_launch(cur)
            return C.c_void_p(cur.cuda_stream)
        return None

    def close(self):
        if self.h:
            self.b.dll.azsp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- configuration ------------------------------------------------------------------------------
    def set_injection(self, noise=None, uniforms=None):
        """noise float64[G, moves, A], uniforms float64[G, moves, 16] (recorded reference randomness)."""
        m = self.cfg.inject_moves
        n = np.ascontiguousarray(noise, dtype=np.float64) if noise is not None else None
        u = np.ascontiguousarray(uniforms, dtype=np.float64) if uniforms is not None else None
        assert n is None or n.shape == (self.G, m, self.A)
        assert u is None or u.shape == (self.G, m, 16)
        self._ck(self.b.dll.azsp_set_injection(self.h, n.ctypes.data if n is not None else None,
                                               u.ctypes.data if u is not None else None, m), "azsp_set_injection")

    # -- games / environment --------------------------------------------------------------------------
    def reset_games(self):
        self._ck(self.b.dll.azsp_reset_games(self.h, self._stream()), "azsp_reset_games")

    def env_step(self, actions=None, want_obs=False):
        """Standalone env kernels.  actions int[G] (None = export only; -2 no-op, -1 resign).
        Returns dict(board int8[G,N,N], legal int8[G,A], scalars int32[G,ENV_COUNT], obs int8[G,2K+1,N,N] | None) on the host."""
        dev = self.device
        if actions is None:
            ap = None
        else:
            self._actions.copy_(torch.as_tensor(np.asarray(actions, dtype=np.int32)))
            ap = self._actions.data_ptr()
        board = torch.empty((self.G, self.N, self.N), dtype=torch.int8, device=dev)
        legal = torch.empty((self.G, self.A), dtype=torch.int8, device=dev)
        scal = torch.empty((self.G, _abi.ENV_COUNT), dtype=torch.int32, device=dev)
        obs = torch.empty((self.G, self.planes, self.N, self.N), dtype=torch.int8, device=dev) if want_obs else None
        self._ck(self.b.dll.azsp_env_step(self.h, ap, board.data_ptr(), legal.data_ptr(), scal.data_ptr(),
                                          obs.data_ptr() if want_obs else None, self._stream()), "azsp_env_step")
        return dict(board=board.cpu().numpy(), legal=legal.cpu().numpy(), scalars=scal.cpu().numpy(),
                    obs=obs.cpu().numpy() if want_obs else None)

    def set_state(self, slot, board, hist, to_play, steps, ko=-1, last_was_pass=False, caps=(0, 0)):
        """hist: the newest-first history boards, 1..8 of them (an env with num_stack K keeps K); a shorter history is padded with
        empty boards to the engine's 8 rows, which an observation of K planes pairs never reads past row K - 1."""
        b = np.ascontiguousarray(board, dtype=np.int8).reshape(-1)
        h = np.asarray(hist, dtype=np.int8).reshape(-1, b.size)
        if not 1 <= h.shape[0] <= 8:
            raise ValueError(f"set_state takes 1..8 history boards, got {h.shape[0]}")
        if h.shape[0] < 8:
            h = np.concatenate([h, np.zeros((8 - h.shape[0], b.size), dtype=np.int8)])
        h = np.ascontiguousarray(h)
        self._ck(self.b.dll.azsp_set_state(self.h, slot, b.ctypes.data, h.ctypes.data, int(to_play), int(steps), int(ko),
                                           int(bool(last_was_pass)), int(caps[0]), int(caps[1]), self._stream()), "azsp_set_state")

    # -- many caller-supplied positions at once (azsp_set_states / azsp_begin_moves / azsp_read_searches) --------------
    def _dev_tensor(self, x, dtype, shape):
        """`x` as one contiguous tensor of `dtype` and `shape` on the engine's device (a host array is copied there once)."""
        t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
        t = t.to(device=self.device, dtype=dtype).contiguous()
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"expected a tensor of shape {tuple(shape)}, got {tuple(t.shape)}")
        return t

    def set_states(self, boards, hist, pos):
        """One launch loads / keeps / idles every slot (azsp_set_states).  boards int8[G, N, N] and hist int8[G, H, N, N] (newest first,
        1 <= H <= 8) in reference colour ids, pos int32[G, PS_COUNT] (_abi.PS_*; column PS_ACTION holds _abi.PSA_LOAD / PSA_KEEP /
        PSA_IDLE): tensors on the engine's device, or host arrays that are copied there once.  Returns the result codes int32[G]
        (_abi.SS_*) as a device tensor; nothing is synchronised."""
        hb = hist.shape[1] if hasattr(hist, "shape") and len(hist.shape) >= 2 else 0
        if not 1 <= hb <= 8:
            raise ValueError(f"set_states takes 1..8 history boards per slot, got {hb}")
        b = self._dev_tensor(boards, torch.int8, (self.G, self.N, self.N))
        h = self._dev_tensor(hist, torch.int8, (self.G, hb, self.N, self.N))
        p = self._dev_tensor(pos, torch.int32, (self.G, _abi.PS_COUNT))
        res = torch.empty((self.G,), dtype=torch.int32, device=self.device)
        self._ck(self.b.dll.azsp_set_states(self.h, b.data_ptr(), h.data_ptr(), hb, p.data_ptr(), res.data_ptr(), self._stream()), "azsp_set_states")
        return res

    def begin_moves(self, noise=None, warm=None):
        """Per-slot begin_move (azsp_begin_moves): noise float64[G, A] or None, warm int32[G] (1 / 0 = the slot's warm_up flag, -1 = derive
        from its steps, _abi.BM_SKIP = leave the slot alone; None = -1 everywhere).  Device tensors, or host arrays copied once."""
        n = self._dev_tensor(noise, torch.float64, (self.G, self.A)) if noise is not None else None
        w = self._dev_tensor(warm if warm is not None else np.full(self.G, -1, dtype=np.int32), torch.int32, (self.G,))
        self._ck(self.b.dll.azsp_begin_moves(self.h, n.data_ptr() if n is not None else None, w.data_ptr(), self._stream()), "azsp_begin_moves")

    def read_searches(self):
        """The last finished search of every slot as DEVICE tensors (azsp_read_searches; nothing is synchronised):
        (pi float64[G, A], child_N float32[G, A], q float64[G, STQ_COUNT], status int32[G, STC_COUNT])."""
        pi = torch.empty((self.G, self.A), dtype=torch.float64, device=self.device)
        cn = torch.empty((self.G, self.A), dtype=torch.float32, device=self.device)
        q = torch.empty((self.G, _abi.STQ_COUNT), dtype=torch.float64, device=self.device)
        st = torch.empty((self.G, _abi.STC_COUNT), dtype=torch.int32, device=self.device)
        self._ck(self.b.dll.azsp_read_searches(self.h, pi.data_ptr(), cn.data_ptr(), q.data_ptr(), st.data_ptr(), self._stream()), "azsp_read_searches")
        return pi, cn, q, st

    # -- search ---------------------------------------------------------------------------------------
    def begin_move(self, noise=None, warm_up=-1):
        n = np.ascontiguousarray(noise, dtype=np.float64).reshape(self.G, self.A) if noise is not None else None
        self._ck(self.b.dll.azsp_begin_move(self.h, n.ctypes.data if n is not None else None, int(warm_up), self._stream()), "azsp_begin_move")

    def select(self, g0=None, g1=None):
        """Select the next leaves of all games, or (g0, g1 given, g0 % 32 == 0) of the games [g0, g1) only."""
        if g0 is None:
            self._ck(self.b.dll.azsp_select(self.h, self.features.data_ptr(), self.valid.data_ptr(), self._stream()), "azsp_select")
        else:
            self._ck(self.b.dll.azsp_select_range(self.h, self.features.data_ptr(), self.valid.data_ptr(), g0, g1, self._stream()), "azsp_select_range")

    def expand_backup(self, g0=None, g1=None):
        if g0 is None:
            self._ck(self.b.dll.azsp_expand_backup(self.h, self.priors.data_ptr(), self.values.data_ptr(), self._stream()), "azsp_expand_backup")
        else:
            self._ck(self.b.dll.azsp_expand_backup_range(self.h, self.priors.data_ptr(), self.values.data_ptr(), g0, g1, self._stream()),
                     "azsp_expand_backup_range")

    def round(self):
        """expand/backup with the current priors/values, then select the next leaves into features/valid."""
        self._ck(self.b.dll.azsp_round(self.h, self.priors.data_ptr(), self.values.data_ptr(), self.features.data_ptr(),
                                       self.valid.data_ptr(), self._stream()), "azsp_round")

    def status(self):
        st = np.zeros((self.G, _abi.STC_COUNT), dtype=np.int32)
        q = np.zeros((self.G, _abi.STQ_COUNT), dtype=np.float64)
        self._ck(self.b.dll.azsp_get_status(self.h, st.ctypes.data, q.ctypes.data, self._stream()), "azsp_get_status")
        return st, q

    def dropin_step(self, priors=None, values=None, feature_rows=None):
        """One iteration of uct_search's simulation loop in ONE host round trip (azsp_dropin_step): upload eval_func's `priors`
        float32[rows, A] / `values` float32[rows] for the previous leaves (None on the first call of a search), expand / backup, select
        the next leaves, and return (status int32[G, STC_COUNT], q float64[G, STQ_COUNT], valid bool[rows], obs [feature_rows, 2K+1, N, N] of the engine's
        feature dtype).  Feature dtypes with a plain [rows, 2K+1, N, N] tensor only (AZSP_FEAT_I8 / F32)."""
        assert not (self.features_tiled or self.features_split)
        nrow = self.rows if feature_rows is None else int(feature_rows)
        if getattr(self, "_dropin_bufs", None) is None:
            np_dt = {torch.int8: np.int8, torch.float32: np.float32}[self.features.dtype]
            self._dropin_bufs = (np.zeros((self.G, _abi.STC_COUNT), dtype=np.int32), np.zeros((self.G, _abi.STQ_COUNT), dtype=np.float64), np.zeros(self.rows, dtype=np.uint8),
                                 np.zeros((self.rows, self.planes, self.N, self.N), dtype=np_dt))
        st, q, valid, obs = self._dropin_bufs
        pp = vp = None
        if priors is not None:
            priors = np.ascontiguousarray(priors, dtype=np.float32).reshape(self.rows, self.A)
            values = np.ascontiguousarray(values, dtype=np.float32).reshape(self.rows)
            pp, vp = priors.ctypes.data, values.ctypes.data
        self._ck(self.b.dll.azsp_dropin_step(self.h, pp, vp, self.priors.data_ptr(), self.values.data_ptr(), self.features.data_ptr(),
                                             self.valid.data_ptr(), st.ctypes.data, q.ctypes.data, valid.ctypes.data, obs.ctypes.data,
                                             nrow * obs[0].nbytes, self._stream()), "azsp_dropin_step")
        return st.copy(), q.copy(), valid.astype(bool), obs[:nrow].copy()  # copies: eval_func may keep what it is handed (the reference passes fresh arrays)

    def get_search(self, slot, ply=0):
        pi = np.zeros(self.A, dtype=np.float64)
        cn = np.zeros(self.A, dtype=np.float32)
        q = np.zeros(_abi.SQ_COUNT, dtype=np.float64)
        self._ck(self.b.dll.azsp_get_search(self.h, slot, ply, pi.ctypes.data, cn.ctypes.data, q.ctypes.data, self._stream()), "azsp_get_search")
        return pi, cn, q

    def commit_move(self, moves):
        m = np.ascontiguousarray(moves, dtype=np.int32).reshape(self.G)
        self._ck(self.b.dll.azsp_commit_move(self.h, m.ctypes.data, self._stream()), "azsp_commit_move")

    def set_actor_state(self, resign_threshold, training_steps):
        """Values every game that STARTS from now on reads (pipeline.py:232-246: the reference actor re-reads the shared resign
        threshold and the checkpoint's training_steps before each game); games in progress keep theirs."""
        self._ck(self.b.dll.azsp_set_actor_state(self.h, C.c_double(float(resign_threshold)), int(training_steps)), "azsp_set_actor_state")

    def set_budgets(self, budgets):
        """Per-slot simulations per move (azsp_set_budgets): int[G], each 1..num_simulations, or 0 = the engine's num_simulations -- the
        node pool and the pb_c tables are sized from it, so it is the upper limit.  A device tensor, or a host array copied once.
        Sticky until the next call; a slot that is mid-search uses its new value at its next budget check.  Nothing is synchronised."""
        if not isinstance(budgets, torch.Tensor):
            budgets = np.asarray(budgets)
            if budgets.shape != (self.G,) or budgets.dtype.kind not in "iu":
                raise ValueError(f"set_budgets takes one integer per slot ({self.G}), got shape {budgets.shape} of {budgets.dtype}")
            if budgets.min() < 0 or budgets.max() > self.cfg.num_simulations:
                raise ValueError(f"a slot's simulations must lie in 1..{self.cfg.num_simulations} (the engine's num_simulations; 0 = that "
                                 f"value), got {int(budgets.min())}..{int(budgets.max())}")
        b = self._dev_tensor(budgets, torch.int32, (self.G,))
        self._ck(self.b.dll.azsp_set_budgets(self.h, b.data_ptr(), self._stream()), "azsp_set_budgets")

    def set_playout_cap(self, fast_simulations, full_prob=1.0):
        """Playout-cap randomisation of the batched actor (azsp_set_playout_cap; not in drop-in mode): every move that starts from now
        on is a full search (the slot's budget, root noise as configured) with probability `full_prob`, else a fast one of
        `fast_simulations` (1..num_simulations) without root noise.  fast_simulations = 0 turns the cap off."""
        self._ck(self.b.dll.azsp_set_playout_cap(self.h, int(fast_simulations), C.c_double(float(full_prob))), "azsp_set_playout_cap")

    def set_leaf_symmetry(self, mode):
        """Leaf symmetry (azsp_set_leaf_symmetry; the reference search has none): None = off, "random" = every feature row is written
        under a dihedral op drawn for it, an integer 0..7 = under that op; the row's priors are mapped back when its node is expanded, the
        value is used as it is.  Holds for the rows selected from now on; rows in flight keep their op.  Samples, logs and env_step
        observations stay in the true orientation."""
        self._ck(self.b.dll.azsp_set_leaf_symmetry(self.h, leaf_symmetry_mode(mode)), "azsp_set_leaf_symmetry")

    def leaf_symmetries(self):
        """uint8[rows] on the engine's device: the op each feature row of the last select was written with (azsp_leaf_symmetries; 0 for
        rows it did not write and with the mode off).  Nothing is synchronised."""
        ops = torch.empty((self.rows,), dtype=torch.uint8, device=self.device)
        self._ck(self.b.dll.azsp_leaf_symmetries(self.h, ops.data_ptr(), self._stream()), "azsp_leaf_symmetries")
        return ops

    def set_forced_playouts(self, k, prune_target=True):
        """Forced playouts at the root with policy-target pruning (azsp_set_forced_playouts; KataGo, Wu 2019, 3.2; the reference search
        has none): None or 0 = off, k > 0 = every root child in play gets at least sqrt(k P(c) sum N) visits in a search that is no fast
        move of the playout cap.  prune_target: the pi recorded for the sample and `target_policies()` leave out the forced visits the
        search did not want; False forces without pruning.  The move, the logs and `read_searches` stay those of the unpruned search.
        Holds for the selections and move ends from now on."""
        kk = forced_playouts_k(k)
        if kk > 0.0 and self._gumbel_m > 0:
            raise ValueError(EXCLUSIVE)
        self._ck(self.b.dll.azsp_set_forced_playouts(self.h, C.c_double(kk), int(bool(prune_target))), "azsp_set_forced_playouts")
        self._forced_k = kk
        self.forced_playouts = self.forced_playouts or kk > 0.0

    def set_gumbel(self, gumbel):
        """Gumbel root search (azsp_set_gumbel; Danihelka et al., ICLR 2022; the reference search has none): None or 0 = off, m or
        (m, c_visit, c_scale) = the root's actions are sampled without replacement with Gumbel noise, m at most are considered, the
        simulations are spent on them by sequential halving, and the policy target is softmax(logits + sigma(completed Q)); below the
        root the search stays PUCT.  Dirichlet noise is not applied; the noise rows of `begin_moves` / `set_injection` carry the Gumbel
        draws.  The move is a* (`gumbel_moves()`; the actor plays it), the target `target_policies()` and the harvested pi rows; the
        logs and `read_searches` keep the plain visit policy.  A fast move of the playout cap runs the plain search.  Not together
        with forced playouts (ValueError).  Holds for the searches that begin from now on."""
        m, cv, cs = gumbel_params(gumbel)
        if m > 0 and self._forced_k > 0.0:
            raise ValueError(EXCLUSIVE)
        self._ck(self.b.dll.azsp_set_gumbel(self.h, m, C.c_double(cv), C.c_double(cs)), "azsp_set_gumbel")
        self._gumbel_m = m
        self.gumbel = self.gumbel or m > 0

    def set_fpu_reduction(self, value):
        """First-play urgency reduction (azsp_set_fpu; Leela Zero, KataGo; the reference search scores an unvisited child as a draw):
        None = off, r or (r_tree, r_root) = at a node with value Q = W / N an unvisited child takes Q - r sqrt(sum of the priors of the
        visited children) in place of -q, with r_root at the root of the search and r_tree below it; 0 is on (the parent's value).  A
        visited child, the u term, the mask and the tie-break are untouched.  Holds for the selections from now on, a search in progress
        included; fast moves of the playout cap follow it, a Gumbel root does below the root."""
        on, rt, rr = fpu_params(value)
        self._ck(self.b.dll.azsp_set_fpu(self.h, on, C.c_double(rt), C.c_double(rr)), "azsp_set_fpu")
        self.fpu_reduction = (rt, rr) if on else None

    def set_aux_targets(self, on=True):
        """Auxiliary training targets per sample (azsp_set_aux_targets; KataGo, Wu 2019, 4.1; the reference actor has none): the
        engine stages the root value of every recorded move and the ownership of every point in the game's final position, and
        `harvest(with_aux=True)` hands out ownership, score and root value in the mover's perspective.  The batched actor only
        (an AzspError on a stop_after_move engine).  Holds for the moves recorded and the games finished from now on; what was staged
        with it off reads 0.  Samples, game rows, logs and searches are untouched."""
        self._ck(self.b.dll.azsp_set_aux_targets(self.h, int(bool(on))), "azsp_set_aux_targets")
        self.aux_targets = self.aux_targets or bool(on)

    def set_policy_surprise(self, value):
        """Policy surprise weighting (azsp_set_policy_surprise; KataGo, Wu 2019; the reference actor has none).  value: None = off, frac
        in [0, 1] or (frac, include_fast), policy_surprise_params.  On, the engine stages with every recorded move the KL divergence
        of its policy target from the root's raw prior, and `harvest(with_surprise=True)` hands out that surprise and the weight of
        every row: a share 1 - frac of a game's full-search rows spread evenly over them, a share frac over the rows in proportion
        to their surprise (with include_fast the fast moves of a playout cap too).  The batched actor only (an AzspError on a
        stop_after_move engine).  On / off holds for the moves recorded from now on (what was staged with it off reads 0, and a game
        without surprise is weighted `full`); frac and include_fast hold for the harvests from now on.  Samples, game rows, logs and
        searches are untouched."""
        on, frac, fast = policy_surprise_params(value)
        self._ck(self.b.dll.azsp_set_policy_surprise(self.h, on, frac, fast), "azsp_set_policy_surprise")
        self.policy_surprise = self.policy_surprise or bool(on)

    def set_visit_reduction(self, value):
        """Decided-game visit reduction (azsp_set_visit_reduction; KataGo's reduceVisits; the reference actor has none).  value: None = off
        or (threshold, lookback, min_simulations, min_weight), visit_reduction_params.  Once one and the same side has led by more than
        `threshold` in the root values of the last `lookback` searches of a game, a full move searches fewer simulations -- down to
        min_simulations as the lead approaches 1 -- and its sample carries a base weight down to min_weight, which
        `harvest(with_base=True)` hands out with the weight of every row.  The batched actor only (ValueError for a malformed value, an
        AzspError on a stop_after_move engine).  Holds for the moves that start from now on; turning it on starts every game's history
        over.  include/azsp.h states the rule."""
        look, t, sims, w = visit_reduction_params(value, self.cfg.num_simulations)
        self._ck(self.b.dll.azsp_set_visit_reduction(self.h, look, t, sims, w), "azsp_set_visit_reduction")
        self.visit_reduction = self.visit_reduction or look > 0

    def gumbel_moves(self):
        """int32[G] on the engine's device: a* of every slot's last finished Gumbel root search, -1 before the first and after a fast move
        (azsp_read_gumbel_moves).  Only once the mode has been enabled.  Nothing is synchronised."""
        out = torch.empty(self.G, dtype=torch.int32, device=self.device)
        self._ck(self.b.dll.azsp_read_gumbel_moves(self.h, out.data_ptr(), self._stream()), "azsp_read_gumbel_moves")
        return out

    def target_policies(self):
        """float64[G, A] on the engine's device: per slot the policy target of its last search that finished with forced playouts or the
        Gumbel root search on (azsp_read_target_policies; zero rows before the first).  Only once one of them has been enabled.  Nothing
        is synchronised."""
        out = torch.empty((self.G, self.A), dtype=torch.float64, device=self.device)
        self._ck(self.b.dll.azsp_read_target_policies(self.h, out.data_ptr(), self._stream()), "azsp_read_target_policies")
        return out

    # -- samples ----------------------------------------------------------------------------------------
    def harvest(self, sample_capacity=None, max_games=None, with_moves=False, with_class=False, with_aux=False, with_surprise=False,
                with_base=False):
        """Returns (states int8[n,2K+1,N,N], pi float32[n,A], z float32[n], games int32[k,GR_COUNT]) -- device tensors + host meta;
        with_moves=True appends moves int16[n] (the move played from every sample's position, -1 = resigned); with_class=True then
        appends full uint8[n] (1 = the sample's move was a full search, 0 = a fast move of the playout cap; all 1 with the cap off).
        with_aux=True (only once aux targets have been enabled) then appends ownership int8[n,N,N] (+1 the mover's point, -1 the
        opponent's, 0 nobody's, in the game's final position), score float32[n] (Go: the final area score with komi seen by the mover;
        Gomoku: z) and root_q float32[n] (the root value of the sample's search): include/azsp.h, azsp_set_aux_targets.
        with_surprise=True (only once policy surprise weighting has been enabled) then appends surprise float32[n] (the KL divergence of
        the sample's policy target from its root's raw prior) and weight float32[n] (how often the row is to be written into the training
        data; DeviceReplay.add_harvest(weights=)): include/azsp.h, azsp_set_policy_surprise.
        with_base=True (only once the visit reduction has been enabled) then appends base float32[n] (the base weight of the sample's
        move, 1.0 unless its search was reduced) and weight float32[n] (as above, with the base in it -- the same tensor if both are
        asked for; base * full with policy surprise off): include/azsp.h, azsp_set_visit_reduction.
        The per-game extras of the same call (azsp_harvest_extra) are left in `self.last_extra` int32[k,GX_COUNT].
        ALIASING: the device tensors are views of buffers this engine re-uses -- the NEXT harvest() overwrites them in place.
        Consume (or .clone()) them before harvesting again; SelfPlayActor.harvest_tensors(clone=True) does the latter."""
        cap = sample_capacity or max(4 * self.G, 2 * self.geo.stage_capacity)
        mg = max_games or 2 * self.G
        if self._harvest_bufs is None or self._harvest_bufs[0].shape[0] < cap:
            self._harvest_bufs = (torch.empty((cap, self.planes, self.N, self.N), dtype=torch.int8, device=self.device),
                                  torch.empty((cap, self.A), dtype=torch.float32, device=self.device),
                                  torch.empty((cap,), dtype=torch.float32, device=self.device),
                                  torch.empty((cap,), dtype=torch.int16, device=self.device),
                                  torch.empty((cap,), dtype=torch.uint8, device=self.device))
        st, pi, z, mvbuf, clbuf = self._harvest_bufs
        self._ck(self.b.dll.azsp_harvest_moves(self.h, mvbuf.data_ptr() if with_moves else None), "azsp_harvest_moves")
        self._ck(self.b.dll.azsp_harvest_search_class(self.h, clbuf.data_ptr() if with_class else None), "azsp_harvest_search_class")
        if with_aux or self._harvest_aux_bufs is not None:  # (an engine that never asked for them makes no call: its harvest is what it was)
            if with_aux and (self._harvest_aux_bufs is None or self._harvest_aux_bufs[0].shape[0] < st.shape[0]):
                self._harvest_aux_bufs = (torch.empty((st.shape[0], self.N, self.N), dtype=torch.int8, device=self.device),
                                          torch.empty((st.shape[0],), dtype=torch.float32, device=self.device),
                                          torch.empty((st.shape[0],), dtype=torch.float32, device=self.device))
            self._ck(self.b.dll.azsp_harvest_aux(self.h, *([t.data_ptr() for t in self._harvest_aux_bufs] if with_aux else [None] * 3)),
                     "azsp_harvest_aux")
        if with_base and (self._harvest_base_bufs is None or self._harvest_base_bufs[0].shape[0] < st.shape[0]):
            self._harvest_base_bufs = tuple(torch.empty((st.shape[0],), dtype=torch.float32, device=self.device) for _ in range(2))
        if with_surprise or self._harvest_surprise_bufs is not None:  # (as above: no call from an engine that never asked)
            if with_surprise and (self._harvest_surprise_bufs is None or self._harvest_surprise_bufs[0].shape[0] < st.shape[0]):
                self._harvest_surprise_bufs = tuple(torch.empty((st.shape[0],), dtype=torch.float32, device=self.device) for _ in range(2))
            if self._harvest_base_bufs is None:  # (an engine that asked for a base registers all three outputs below)
                self._ck(self.b.dll.azsp_harvest_surprise(self.h, *([t.data_ptr() for t in self._harvest_surprise_bufs] if with_surprise else [None] * 2)),
                         "azsp_harvest_surprise")
        weight = None
        if self._harvest_base_bufs is not None:
            weight = self._harvest_surprise_bufs[1] if with_surprise else (self._harvest_base_bufs[1] if with_base else None)
            self._ck(self.b.dll.azsp_harvest_weights(self.h, self._harvest_surprise_bufs[0].data_ptr() if with_surprise else None,
                                                     weight.data_ptr() if weight is not None else None,
                                                     self._harvest_base_bufs[0].data_ptr() if with_base else None), "azsp_harvest_weights")
        games = np.zeros((mg, _abi.GR_COUNT), dtype=np.int32)
        extra = np.zeros((mg, _abi.GX_COUNT), dtype=np.int32)
        self._ck(self.b.dll.azsp_harvest_extra(self.h, extra.ctypes.data), "azsp_harvest_extra")
        ns, ng = C.c_int32(0), C.c_int32(0)
        self._ck(self.b.dll.azsp_harvest(self.h, st.data_ptr(), pi.data_ptr(), z.data_ptr(), st.shape[0], games.ctypes.data, mg,
                                         C.byref(ns), C.byref(ng), self._stream()), "azsp_harvest")
        n, k = ns.value, ng.value
        self._ck(self.b.dll.azsp_harvest_extra(self.h, None), "azsp_harvest_extra")  # the host array dies with this call
        self.last_extra = extra[:k]
        out = (st[:n], pi[:n], z[:n], games[:k])
        if with_moves:
            out += (mvbuf[:n],)
        if with_class:
            out += (clbuf[:n],)
        if with_aux:
            out += tuple(t[:n] for t in self._harvest_aux_bufs)
        if with_surprise:
            out += tuple(t[:n] for t in self._harvest_surprise_bufs)
        if with_base:
            out += (self._harvest_base_bufs[0][:n], weight[:n])
        return out

    def counters(self, reset=False):
        out = np.zeros(16, dtype=np.uint64)
        self._ck(self.b.dll.azsp_counters(self.h, out.ctypes.data, int(reset), self._stream()), "azsp_counters")
        return {k: int(out[i]) for i, k in enumerate(_abi.COUNTER_NAMES)}
