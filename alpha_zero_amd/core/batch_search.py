"""Search many caller-supplied positions at once: `BatchSearch` (one engine, one wavefront per position).

The drop-in `uct_search` (core/mcts_v2.py) builds a ONE-game engine per search; a caller who brings n positions -- an opening book, a
puzzle or regression suite, positions out of SGF collections, a match resumed in the middle -- pays n sequential searches.  A
`BatchSearch` owns one engine in drop-in mode (`stop_after_move`) with `capacity` slots and searches up to `capacity` positions in
lock-step: one `azsp_set_states` launch loads them all from device tensors, one `azsp_begin_moves` hands every slot its own Dirichlet
draw and `warm_up` flag, the simulation loop evaluates the leaves of ALL slots in one batch, and `azsp_read_searches` returns every
slot's pi / child_N / Q as device tensors.  Every slot's search is the search `uct_search` would run on that position alone (games
never interact inside the engine, mcts_v2.py:568-625 is per game): same moves, pi and Q, bit for bit, with an evaluator whose outputs
do not depend on the batch a row arrives in (tests/batch_search_checks.py).

Per-position arguments and results (noise rows, warm flags, `results()`, `commit`) follow `self.slots`: the active slots in ascending
order.
"""
import numpy as np
import torch

from .. import _abi
from ..envs.base import BoardGameEnv
from .engine import Engine, EngineConfig, SearchOptions


def dropin_engine(game, board_size, num_games, num_simulations, num_parallel, c_puct_base, c_puct_init, root_noise, komi=7.5, max_steps=0,
                  num_to_win=5, num_stack=8, binding=None, device=None, leaf_symmetry=None, forced_playouts=None, gumbel=None,
                  fpu_reduction=None):
    """The engine of a drop-in search, `uct_search`'s with one game and a BatchSearch's with `capacity`: it stops after every move
    (`stop_after_move`), hands out int8 observation planes and logs no moves.  Without a `binding` it runs the product library on the GPU.
    leaf_symmetry, forced_playouts, gumbel, fpu_reduction: SearchOptions.of."""
    SearchOptions.of(leaf_symmetry, forced_playouts, gumbel=gumbel, fpu_reduction=fpu_reduction)  # ValueError before anything is built
    if binding is None:
        from .. import _lib

        binding, device = _lib.load(require_gpu=True), device or "cuda"
    cfg = EngineConfig(game=game, board_size=board_size, num_games=num_games, num_parallel=num_parallel, num_simulations=num_simulations,
                       c_puct_base=c_puct_base, c_puct_init=c_puct_init, root_noise=root_noise, komi=komi, max_steps=max_steps or 0,
                       num_to_win=num_to_win, num_stack=num_stack, stop_after_move=True, feature_dtype=_abi.FEAT_I8, log_moves=False,
                       leaf_symmetry=leaf_symmetry, forced_playouts=forced_playouts, gumbel=gumbel, fpu_reduction=fpu_reduction)
    return Engine(binding, cfg, device=device)


def env_settings(env):
    """The keyword arguments of `dropin_engine` / `BatchSearch` that are read off an env: its game, rules and backend."""
    return dict(game="go" if env.has_pass_move else "gomoku", board_size=env.board_size, komi=getattr(env, "komi", 7.5),
                max_steps=getattr(env, "max_steps", 0) or 0, num_to_win=getattr(env, "num_to_win", 5), num_stack=getattr(env, "num_stack", 8),
                binding=getattr(env, "_binding", None), device=getattr(env, "_device", None))


def check_env(env):
    if not isinstance(env, BoardGameEnv) and not (hasattr(env, "board_deltas") and hasattr(env, "legal_actions")):
        raise ValueError(f"Expect `env` to be a valid BoardGameEnv instance, got {env}")


def check_num_simulations(num_simulations):
    if not 1 <= num_simulations:
        raise ValueError(f"Expect `num_simulations` to a positive integer, got {num_simulations}")


def slot_simulations(num_simulations, n, limit):
    """int64[n]: `num_simulations` -- an int for all, or a sequence of n ints -- as one number of simulations per active slot of a
    search whose engine was built for `limit`.  ValueError for a wrong length or a value outside 1..limit (the engine's node pool and
    pb_c tables are sized from `limit`)."""
    a = np.asarray(num_simulations)
    if a.dtype.kind not in "iu" or a.ndim > 1 or (a.ndim == 1 and a.shape[0] != n):
        raise ValueError(f"`num_simulations` must be an integer or one integer per active slot ({n}), got {num_simulations!r}")
    a = np.broadcast_to(a.astype(np.int64), (n,))
    if n and (a.min() < 1 or a.max() > limit):
        raise ValueError(f"`num_simulations` of a slot must lie in 1..{limit} (what this search's engine was built for), got "
                         f"{int(a.min())}..{int(a.max())}")
    return a


def check_planes(eval_func, planes, num_stack):
    cin = getattr(eval_func, "in_channels", None)  # known for evaluators that wrap a network (core/evaluate.py DeviceEvaluator)
    if cin is not None and cin != planes:
        raise ValueError(f"the evaluator's network takes {cin} input planes, but the observations (num_stack = {num_stack}) have {planes}")


def evaluator_device(eval_func):
    """The device an evaluator's network lives on: its `device` attribute, else the device of the parameters of its `inf` module
    (core/evaluate.py DeviceEvaluator); None when it cannot be told."""
    dev = getattr(eval_func, "device", None)
    if dev is not None:
        return torch.device(dev)
    inf = getattr(eval_func, "inf", None)
    try:
        return next(inf.parameters()).device if inf is not None else None
    except (StopIteration, AttributeError, TypeError):
        return None


def is_resident(eval_func, eng):
    """True when `eval_func` can run between the engine's own tensors (the resident loop): it has `device_eval` / `device_eval_into`, the
    engine's features are a plain tensor, and the evaluator is not known to live on another device than the engine (an evaluator that
    does falls back to the host callback loop, which moves the rows itself)."""
    if getattr(eval_func, "device_eval", None) is None and getattr(eval_func, "device_eval_into", None) is None:
        return False
    if eng.features_tiled or eng.features_split:
        return False
    dev = evaluator_device(eval_func)
    if dev is None:
        return True
    fd = eng.features.device
    return dev.type == fd.type and (dev.index is None or fd.index is None or dev.index == fd.index)


def env_key(env):
    """What must agree between the envs of one batch (and the engine that searches them)."""
    go = bool(env.has_pass_move)
    return _key("go" if go else "gomoku", env.board_size, getattr(env, "komi", 7.5), getattr(env, "max_steps", 0), getattr(env, "num_to_win", 5),
                getattr(env, "num_stack", 8))


def _key(game, n, komi, max_steps, num_to_win, num_stack):
    go = game == "go"  # (max_steps 0 = the default 2 N^2, go.py:48; komi / max_steps mean nothing at Gomoku, num_to_win nothing at Go)
    return (game, int(n), float(komi) if go else None, int(max_steps or 2 * n * n) if go else None, None if go else int(num_to_win), int(num_stack))


def env_position(env):
    """(board int8[N, N], hist int8[K, N, N] newest first, pos row int32[PS_COUNT] with action LOAD) of an env: the one reader of an
    env's position, for the single search (core/mcts_v2.py _load_position) and the batched one.  K = env.num_stack rows (a reference
    env's deque); the engine pads them to its 8."""
    hist = np.stack([np.asarray(b, dtype=np.int8) for b in env.board_deltas])
    ko, caps = getattr(env, "ko", -1), getattr(env, "_caps", (0, 0))
    p = getattr(env, "position", None)  # a reference GoEnv keeps these on its Position
    if p is not None:
        ko = -1 if p.ko is None else p.ko[0] * env.board_size + p.ko[1]
        caps = tuple(p.caps)
    last_pass = bool(env.has_pass_move and len(env.history) > 0 and env.history[-1].move == env.pass_move)
    row = np.zeros(_abi.PS_COUNT, dtype=np.int32)
    row[[_abi.PS_ACTION, _abi.PS_TO_PLAY, _abi.PS_STEPS, _abi.PS_KO, _abi.PS_LAST_PASS, _abi.PS_CAPS_BLACK, _abi.PS_CAPS_WHITE]] = (
        _abi.PSA_LOAD, env.to_play, env.steps, ko, int(last_pass), caps[0], caps[1])
    return np.asarray(env.board, dtype=np.int8), hist, row


def simulate_with_callback(eng, eval_func, slots, num_parallel=None):
    """The simulation loop (mcts_v2.py:378-421 / :568-625) of the searches in `slots` with the caller's HOST callback.  One host round
    trip per leaf batch: azsp_dropin_step uploads eval_func's outputs, runs expand / backup + the selection of the next leaves, and
    returns status, valid flags and the leaves' observation planes from one packed read-back (rounds 1-5 paid eight stream
    synchronisations per simulation here).

    num_parallel says how the valid leaf rows reach `eval_func`.  None, the batched searches: always ONE eval_func(obs[rows], True) for
    the rows of all slots.  A number, the single search of slot 0 (`uct_search` with 1, `parallel_uct_search` with its P): the
    reference's calls, unbatched for a root evaluation and for every leaf of uct_search."""
    pri = np.zeros((eng.rows, eng.A), dtype=np.float32)
    val = np.zeros(eng.rows, dtype=np.float32)
    st, _, valid, obs = eng.dropin_step(None, None)
    for _ in range(1 << 20):
        if all(st[s, _abi.STC_STATUS] == _abi.ST_MOVE_DONE for s in slots):  # (scalar reads: np.all over st[slots] cost uct_search 6 % of its moves/s with a free evaluator)
            return
        if valid.any():
            if num_parallel is not None and (st[0, _abi.STC_ROOT_EVAL_PENDING] or num_parallel == 1):  # mcts_v2.py:365, :414, :555
                p, v = eval_func(obs[0], False)
                pri[0], val[0] = np.asarray(p, dtype=np.float32), v
            else:
                rows = np.flatnonzero(valid)
                ps, vs = eval_func(obs[rows], True)  # mcts_v2.py:614 per game
                for r, p, v in zip(rows, ps, vs):
                    pri[r], val[r] = np.asarray(p, dtype=np.float32), v
        st, _, valid, obs = eng.dropin_step(pri, val)
    raise RuntimeError("the searches did not finish")


def simulate_on_device(eng, evaluator, num_simulations, num_parallel, slots):
    """The same loop for an evaluator that lives on the engine's device (anything with `device_eval(x) -> (priors, values)` on device
    tensors, e.g. core/evaluate.py DeviceEvaluator): select writes the leaves' observation planes into `eng.features`, the evaluator reads
    them there and its outputs go straight into `eng.priors` / `eng.values`, expand / backup reads those -- NO host round trip per
    simulation.  The host only polls the status rows of `slots`: a search that still owes `left` simulations cannot finish in fewer than
    left / (simulations one iteration can complete) iterations (1 for uct_search -- a terminal leaf makes select descend again in the
    same launch, mcts_v2.py:378-411 --, at most 2P attempts for parallel_uct_search, :572), so that many iterations are queued without
    looking (half of them: a search with terminal leaves needs fewer, and iterations queued after the search is done would be no-ops in
    the engine -- nothing pending, status MOVE_DONE -- but each still costs a forward).  ~8 polls per 100-simulation move instead of 100
    round trips.  With several slots the queue is sized by the slot that owes the most: a finished slot ignores rounds.  Every row is
    evaluated, valid or not, like the batched actor does: the engine ignores outputs of rows it did not ask for.  Same searches as the
    callback loop with the same evaluator (tests/dropin_checks.py).  num_simulations: an int, or one per entry of `slots` (per-slot
    budgets, Engine.set_budgets): what a pending slot still owes is counted against its own number."""
    sims = np.broadcast_to(np.asarray(num_simulations, dtype=np.int64), (len(slots),))
    per_iter = 1 if num_parallel == 1 else 2 * num_parallel
    into = getattr(evaluator, "device_eval_into", None)
    eng.round()  # nothing to back up yet: selects the first leaves (or asks for the roots' evaluations)
    for _ in range(1 << 20):
        st, _ = eng.status()
        rows = st[slots]
        pending = rows[:, _abi.STC_STATUS] != _abi.ST_MOVE_DONE
        if not pending.any():
            return
        left = max(int((sims[pending] - rows[pending, _abi.STC_ROOT_N]).max()), 1)
        for _ in range(max(1, (left // 2) // per_iter)):
            if into is not None:
                into(eng.features, eng.priors, eng.values)
            else:
                pri, val = evaluator.device_eval(eng.features)
                eng.priors.copy_(pri.reshape(eng.priors.shape))
                eng.values.copy_(val.reshape(eng.values.shape))
            eng.round()
    raise RuntimeError("the searches did not finish")


def choose_move(env, search_pi, child_n, root_legal, warm_up, deterministic):
    """The move of a finished search (mcts_v2.py:427-434 / :634-641): the most visited child, or `np.random.choice` draws from `search_pi` until
    the move is legal and, in the warm-up phase, no pass."""
    move = None
    if deterministic:
        move = np.argmax(child_n)
    else:
        while move is None or (warm_up and env.has_pass_move and move == env.pass_move) or root_legal[move] != 1:
            move = np.random.choice(np.arange(search_pi.shape[0]), p=search_pi)
    assert root_legal[move] == 1
    return move


class SearchResults:
    """`BatchSearch.results()`: device tensors, one row per active slot; `.cpu()` returns pi, child_N and root_Q as NumPy arrays.
    target_pi: None, or with forced playouts on float64[n, A], the pruned policy target of every slot's search (pi stays unpruned); with
    the Gumbel root search on, the completed-Q target pi'.  gumbel_move: None, or with the Gumbel root search on int32[n], the move a*
    of every slot's search -- the one to commit."""

    def __init__(self, pi, child_N, root_Q, target_pi=None, gumbel_move=None):
        self.pi, self.child_N, self.root_Q, self.target_pi, self.gumbel_move = pi, child_N, root_Q, target_pi, gumbel_move

    def cpu(self):
        return self.pi.cpu().numpy(), self.child_N.cpu().numpy(), self.root_Q.cpu().numpy()


class BatchSearch:
    """One engine with `capacity` slots that searches caller-supplied positions in lock-step; reused across calls.

    load / load_envs  ->  search  ->  results  ->  commit  -> (load the slots that lost their tree again) -> search ...
    """

    def __init__(self, game, board_size, capacity, num_simulations, num_parallel=1, c_puct_base=19652.0, c_puct_init=1.25, root_noise=False,
                 komi=7.5, max_steps=0, num_to_win=5, num_stack=8, binding=None, device=None, leaf_symmetry=None, forced_playouts=None,
                 gumbel=None, fpu_reduction=None):
        """leaf_symmetry, forced_playouts, gumbel, fpu_reduction: SearchOptions.of.  What they mean here: with gumbel the move to commit is
        `results().gumbel_move` and the sample to record `results().target_pi`; `search(noise=...)` takes the Gumbel(0, 1) rows (None:
        drawn here with np.random.gumbel) and root_noise is ignored.  With forced_playouts the move is still to be chosen from
        `results().pi`, the sample to record is `results().target_pi` (None when both are off).  Under leaf_symmetry `eval_func` --
        host callback or resident evaluator -- is handed every leaf position under that board symmetry."""
        opt = SearchOptions.of(leaf_symmetry, forced_playouts, gumbel=gumbel, fpu_reduction=fpu_reduction)
        if capacity < 1:
            raise ValueError(f"capacity must be at least 1, got {capacity}")
        check_num_simulations(num_simulations)
        self.forced_playouts, self.gumbel = opt.forced_k > 0.0, opt.gumbel[0] > 0
        self.game, self.capacity, self.num_simulations, self.num_parallel = game, int(capacity), int(num_simulations), int(num_parallel)
        self.key = _key(game, board_size, komi, max_steps, num_to_win, num_stack)
        self.eng = dropin_engine(game, board_size, self.capacity, num_simulations, num_parallel, c_puct_base, c_puct_init, root_noise, komi,
                                 max_steps, num_to_win, num_stack, binding, device, leaf_symmetry, forced_playouts, gumbel, fpu_reduction)
        self.slots = np.zeros(0, dtype=np.int64)  # the active slots (a position is loaded, or a sub-tree was kept), ascending
        self._status = np.full(self.capacity, _abi.ST_IDLE, dtype=np.int32)  # host mirror of the slots' status after load / search / commit
        self._budgets_set = False  # an earlier search left per-slot budgets in the engine (search(num_simulations=...))

    @classmethod
    def for_env(cls, env, capacity, num_simulations, num_parallel=1, c_puct_base=19652.0, c_puct_init=1.25, root_noise=False,
                fpu_reduction=None):
        """A BatchSearch for positions of `env`'s game, board size, komi / max_steps / num_to_win and num_stack, on `env`'s backend.
        fpu_reduction: SearchOptions.of."""
        return cls(capacity=capacity, num_simulations=num_simulations, num_parallel=num_parallel, c_puct_base=c_puct_base, c_puct_init=c_puct_init,
                   root_noise=root_noise, fpu_reduction=fpu_reduction, **env_settings(env))

    def close(self):
        if self.eng is not None:
            self.eng.close()
            self.eng = None

    # -- positions ------------------------------------------------------------------------------------
    def _slot_list(self, slots, n):
        s = np.arange(n, dtype=np.int64) if slots is None else np.asarray(slots, dtype=np.int64).reshape(-1)
        if n > self.capacity:
            raise ValueError(f"{n} positions do not fit the {self.capacity} slots of this BatchSearch")
        if len(s) != n or len(set(s.tolist())) != n or (n and (s.min() < 0 or s.max() >= self.capacity)):
            raise ValueError(f"`slots` must name {n} different slots in 0..{self.capacity - 1}, got {s.tolist()}")
        return s

    def load(self, boards, hist, pos, slots=None, keep=()):
        """Position i goes to slot slots[i] (default i): boards int8[n, N, N], hist int8[n, H, N, N] (newest first, 1 <= H <= 8), pos
        int32[n, PS_COUNT] (_abi.PS_*; its ACTION column is set to LOAD here) -- torch tensors on the engine's device, or host arrays
        that are copied there once.  Slots named in `keep` are left as they are (a sub-tree kept by `commit`); every other slot is idled.
        All of it is ONE azsp_set_states launch.  Returns the result codes int32[n] (_abi.SS_OK / SS_INVALID / SS_GAME_OVER); the slots
        that were refused are idle and take no part in the search."""
        eng, G = self.eng, self.capacity
        n = int(boards.shape[0]) if len(boards.shape) == 3 else -1
        if n < 0:
            raise ValueError(f"`boards` must be [n, N, N], got {tuple(boards.shape)}")
        s = self._slot_list(slots, n)
        kp = np.asarray(list(keep), dtype=np.int64).reshape(-1)
        if len(kp) and (kp.min() < 0 or kp.max() >= G or np.intersect1d(kp, s).size or len(set(kp.tolist())) != len(kp)):
            raise ValueError(f"`keep` must name different slots in 0..{G - 1} that are not loaded in the same call, got {kp.tolist()}")
        dev = eng.device
        as_t = lambda x, dt: (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))).to(device=dev, dtype=dt)  # noqa: E731
        b, h, p = as_t(boards, torch.int8), as_t(hist, torch.int8), as_t(pos, torch.int32).clone()
        if h.dim() != 4 or h.shape[0] != n or not 1 <= h.shape[1] <= 8:
            raise ValueError(f"`hist` must be [n, 1..8, N, N], got {tuple(h.shape)}")
        if tuple(p.shape) != (n, _abi.PS_COUNT):
            raise ValueError(f"`pos` must be [n, {_abi.PS_COUNT}], got {tuple(p.shape)}")
        p[:, _abi.PS_ACTION] = _abi.PSA_LOAD
        H = int(h.shape[1])
        if n == G and np.array_equal(s, np.arange(G)):
            fb, fh, fp = b, h, p
        else:  # scatter the n rows into full [G, ...] tensors; the other slots idle, or keep what they have
            idx = torch.from_numpy(s).to(dev)
            fb = torch.zeros((G, eng.N, eng.N), dtype=torch.int8, device=dev).index_copy_(0, idx, b)
            fh = torch.zeros((G, H, eng.N, eng.N), dtype=torch.int8, device=dev).index_copy_(0, idx, h)
            fp = torch.zeros((G, _abi.PS_COUNT), dtype=torch.int32, device=dev)
            fp[:, _abi.PS_ACTION] = _abi.PSA_IDLE
            if len(kp):
                fp[torch.from_numpy(kp).to(dev), _abi.PS_ACTION] = _abi.PSA_KEEP
            fp.index_copy_(0, idx, p)
        res = eng.set_states(fb, fh, fp).cpu().numpy()
        kept = self._status[kp] if len(kp) else np.zeros(0, dtype=np.int32)
        self._status[:] = _abi.ST_IDLE
        self._status[s[res[s] == _abi.SS_OK]] = _abi.ST_NEED_ROOT
        if len(kp):
            self._status[kp] = kept
        self.slots = np.flatnonzero(self._status != _abi.ST_IDLE)
        return res[s]

    def load_envs(self, envs, slots=None, keep=()):
        """`load` for env objects (alpha_zero_amd.envs or the reference's): board, board_deltas, to_play, steps, ko, captures and
        last-pass are read the way the drop-in search reads them; ONE set_states for all of them."""
        envs = list(envs)
        if len(envs) > self.capacity:
            raise ValueError(f"{len(envs)} positions do not fit the {self.capacity} slots of this BatchSearch")
        for env in envs:
            check_env(env)
            if env_key(env) != self.key:
                raise ValueError(f"all envs of a batch must share game, board size, komi / max_steps / num_to_win and num_stack with the "
                                 f"engine: {env_key(env)} != {self.key}")
        for env in envs:
            if env.is_game_over():
                raise RuntimeError("Game is over.")
        if not envs:
            N, K = self.eng.N, self.eng.cfg.num_stack
            return self.load(np.zeros((0, N, N), np.int8), np.zeros((0, K, N, N), np.int8), np.zeros((0, _abi.PS_COUNT), np.int32), slots, keep)
        parts = [env_position(env) for env in envs]
        return self.load(np.stack([x[0] for x in parts]), np.stack([x[1] for x in parts]), np.stack([x[2] for x in parts]), slots, keep)

    # -- search ---------------------------------------------------------------------------------------
    def search(self, eval_func, noise=None, warm_up=False, num_simulations=None):
        """Run every active slot's search to its end (status MOVE_DONE).  noise: float64[len(slots), A] Dirichlet draws or None (with
        `gumbel` on: Gumbel(0, 1) draws; None = drawn here from np.random); warm_up:
        a bool, or one bool per active slot (both in `self.slots` order).  num_simulations: None = this object's own number for every
        slot; an int, or one int per active slot in `self.slots` order, in 1..self.num_simulations = that slot's budget for THIS call
        (a kept sub-tree whose root already has that many visits is done at once, as in the reference's `while root.N < budget`).

        An evaluator with `device_eval_into` / `device_eval` that lives on the engine's device runs the resident loop: the leaves of all
        slots stay on the device, the host polls the status rows a few times per search.  Any other `eval_func` is called on the host:
        every iteration the valid leaf rows of ALL slots go to `eval_func(obs, True)` in ONE call and it returns (priors, values) for
        them -- a batched search needs a batch-capable eval_func.  The reference's unbatched call `eval_func(obs, False)` (P = 1 and
        root evaluations) is the one contract of uct_search this class does not keep."""
        check_planes(eval_func, self.eng.planes, self.eng.cfg.num_stack)
        eng, G, sl = self.eng, self.capacity, self.slots
        sims = self.num_simulations if num_simulations is None else slot_simulations(num_simulations, len(sl), self.num_simulations)
        if len(sl) == 0:
            return
        if num_simulations is not None or self._budgets_set:  # (None also undoes what an earlier call left in the slots)
            b = np.zeros(G, dtype=np.int32)
            b[sl] = 0 if num_simulations is None else sims
            eng.set_budgets(b)
            self._budgets_set = num_simulations is not None
        warm = np.full(G, _abi.BM_SKIP, dtype=np.int32)
        warm[sl] = np.broadcast_to(np.asarray(warm_up, dtype=bool), (len(sl),)).astype(np.int32)
        full_noise = None
        if noise is None and self.gumbel:
            noise = np.random.gumbel(size=(len(sl), eng.A))
        if noise is not None:
            nz = noise if isinstance(noise, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(noise, dtype=np.float64))
            nz = nz.to(device=eng.device, dtype=torch.float64).reshape(len(sl), eng.A)
            full_noise = nz if len(sl) == G else torch.zeros((G, eng.A), dtype=torch.float64, device=eng.device).index_copy_(
                0, torch.from_numpy(sl).to(eng.device), nz)
        eng.begin_moves(full_noise, warm)
        if is_resident(eval_func, eng):
            simulate_on_device(eng, eval_func, sims, self.num_parallel, sl)
        else:
            simulate_with_callback(eng, eval_func, sl)
        self._status[sl] = _abi.ST_MOVE_DONE

    # -- results --------------------------------------------------------------------------------------
    def results(self):
        """(pi, child_N, root_Q) of the active slots' finished searches as DEVICE tensors in a SearchResults (`.cpu()` for NumPy): pi is
        float64 for Go and float32 for Gomoku, as uct_search returns it; child_N float32[n, A]; root_Q float64[n]."""
        pi, cn, q, _ = self.eng.read_searches()
        idx = torch.from_numpy(self.slots).to(self.eng.device)
        pi = pi.index_select(0, idx)
        if self.game != "go":
            pi = pi.to(torch.float32)  # float64 for Go, float32 for Gomoku
        target = self.eng.target_policies().index_select(0, idx) if (self.forced_playouts or self.gumbel) else None
        moves = self.eng.gumbel_moves().index_select(0, idx) if self.gumbel else None
        return SearchResults(pi, cn.index_select(0, idx), q.index_select(0, idx)[:, _abi.STQ_ROOT_Q].contiguous(), target, moves)

    def commit(self, moves):
        """The chosen move of every active slot (`self.slots` order).  Returns (best_child_Q float64[n], reusable bool[n]): a slot whose
        chosen child exists and is not terminal keeps its sub-tree (status SEARCH) and stays active for the next `search`; the others
        are idle and must be loaded again."""
        sl = self.slots
        m = np.full(self.capacity, -1, dtype=np.int32)
        m[sl] = np.asarray(moves, dtype=np.int32).reshape(len(sl))
        self.eng.commit_move(m)
        st, q = self.eng.status()
        self._status[:] = st[:, _abi.STC_STATUS]
        reusable = st[sl, _abi.STC_STATUS] == _abi.ST_SEARCH
        child_q = q[sl, _abi.STQ_CHILD_Q].copy()
        self.slots = np.flatnonzero((self._status != _abi.ST_IDLE))
        return child_q, reusable
