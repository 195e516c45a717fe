"""Drop-in `uct_search` / `parallel_uct_search` (reference: alpha_zero/core/mcts_v2.py:301-657) on the GPU engine.

Same signatures, same return tuple `(move, search_pi, root_Q, best_child_Q, next_root_node)`, same
errors, same use of the global NumPy random state (one `np.random.dirichlet` per call when
`root_noise`, then `np.random.choice` draws until the move is acceptable), so an actor or evaluator
written against the reference runs unchanged.  The tree lives in HBM inside a one-game engine
(stop_after_move mode of the C ABI); `eval_func` is the caller's Python callback and receives the
observation planes the select kernel produced, exactly the arrays the reference would pass it.
`next_root_node` is an opaque handle (callers only pass it back).

`uct_search_many` / `parallel_uct_search_many` are the batched forms: a LIST of envs is searched in lock-step on one engine, one
wavefront per env (core/batch_search.py), and ONE handle carries the sub-trees of the whole batch to the next call.
"""
import weakref

import numpy as np

from .. import _abi
from .batch_search import (BatchSearch, check_env, check_num_simulations, check_planes, choose_move, dropin_engine, env_key, env_position,
                           env_settings, is_resident, simulate_on_device, simulate_with_callback, slot_simulations)

_POOL = {}  # config key -> idle _Searcher objects


class Node:
    """Opaque handle of a re-usable sub-tree (the reference returns its Node object here)."""

    def __init__(self, searcher, board, to_play, steps):
        self._searcher, self._board, self.to_play, self._steps = searcher, board, to_play, steps
        self._alive = True
        # Returns the engine to the pool when a LIVE handle is dropped (the caller abandoned the tree).  A handle that is handed
        # back to the next search passes its engine on to the new handle: its finalizer is detached there, otherwise dropping the
        # old handle would put an engine that is still in use into the pool (and a second search would overwrite the live tree).
        self._fin = weakref.finalize(self, _release, searcher)

    @property
    def is_expanded(self):
        return True


def _release(searcher):
    idle = _POOL.setdefault(searcher.key, [])
    if not any(x is searcher for x in idle):  # never pool the same engine twice
        idle.append(searcher)


class _Searcher:
    def __init__(self, key, env, sims, P, base, init, root_noise):
        self.key = key
        self.eng = dropin_engine(num_games=1, num_simulations=sims, num_parallel=P, c_puct_base=base, c_puct_init=init, root_noise=root_noise,
                                 **env_settings(env))


def _get_searcher(env, sims, P, base, init, root_noise):
    key = ("go" if env.has_pass_move else "gomoku", env.board_size, sims, P, float(base), float(init), bool(root_noise),
           getattr(env, "komi", None), getattr(env, "max_steps", None), getattr(env, "num_to_win", None), getattr(env, "num_stack", 8),
           id(getattr(env, "_binding", None)))
    idle = _POOL.get(key)
    if idle:
        return idle.pop()
    return _Searcher(key, env, sims, P, base, init, root_noise)


def _load_position(s, env):
    board, hist, row = env_position(env)
    s.eng.set_state(0, board, hist, row[_abi.PS_TO_PLAY], row[_abi.PS_STEPS], row[_abi.PS_KO], row[_abi.PS_LAST_PASS],
                    (row[_abi.PS_CAPS_BLACK], row[_abi.PS_CAPS_WHITE]))


def _search(env, eval_func, root_node, c_puct_base, c_puct_init, num_simulations, num_parallel, root_noise, warm_up, deterministic):
    check_env(env)
    check_num_simulations(num_simulations)
    if env.is_game_over():
        raise RuntimeError("Game is over.")
    num_stack = getattr(env, "num_stack", 8)
    check_planes(eval_func, 2 * num_stack + 1, num_stack)
    if root_node is not None:
        if not isinstance(root_node, Node) or not root_node._alive:
            raise ValueError("`root_node` must be the handle returned by the previous search (or None)")
        if root_node.to_play != env.to_play or root_node._steps != env.steps or not np.array_equal(root_node._board, env.board):
            raise ValueError("`root_node` does not belong to this position")
        s = root_node._searcher
        root_node._alive = False
        root_node._fin.detach()  # the engine moves on with this search; only the NEXT handle (or game end) releases it
    else:
        s = _get_searcher(env, num_simulations, num_parallel, c_puct_base, c_puct_init, root_noise)
        _load_position(s, env)
    eng = s.eng
    root_legal = env.legal_actions
    noise = None
    if root_noise:  # add_dirichlet_noise (mcts_v2.py:259-260): the engine applies the legal mask itself
        noise = np.random.dirichlet(np.ones_like(root_legal) * 0.03)
    eng.begin_move(noise, warm_up=1 if warm_up else 0)
    if is_resident(eval_func, eng):
        # a device-resident evaluator (core/evaluate.py DeviceEvaluator): the leaves never visit the host -- see simulate_on_device
        simulate_on_device(eng, eval_func, num_simulations, num_parallel, [0])
    else:
        simulate_with_callback(eng, eval_func, [0], num_parallel)
    pi64, child_n, _ = eng.get_search(0, 0)
    search_pi = pi64 if env.has_pass_move else pi64.astype(np.float32)  # float64 for Go, float32 for Gomoku
    move = choose_move(env, search_pi, child_n, root_legal, warm_up, deterministic)
    eng.commit_move([int(move)])
    st, q = eng.status()
    next_root = None
    if st[0, _abi.STC_STATUS] == _abi.ST_SEARCH:
        out = eng.env_step(None)  # export the new root position for the hand-over check of the next call
        next_root = Node(s, out["board"][0].copy(), int(out["scalars"][0][_abi.ENV_TO_PLAY]), int(out["scalars"][0][_abi.ENV_STEPS]))
    else:
        _release(s)
    return (move, search_pi, float(q[0, _abi.STQ_ROOT_Q]), float(q[0, _abi.STQ_CHILD_Q]), next_root)


def uct_search(env, eval_func, root_node, c_puct_base, c_puct_init, num_simulations=800, root_noise=False, warm_up=False,
               deterministic=False):
    """mcts_v2.py:301-450"""
    return _search(env, eval_func, root_node, c_puct_base, c_puct_init, num_simulations, 1, root_noise, warm_up, deterministic)


def parallel_uct_search(env, eval_func, root_node, c_puct_base, c_puct_init, num_simulations, num_parallel, root_noise=False,
                        warm_up=False, deterministic=False):
    """mcts_v2.py:485-657"""
    return _search(env, eval_func, root_node, c_puct_base, c_puct_init, num_simulations, num_parallel, root_noise, warm_up,
                   deterministic)


# ---------------------------------------------------------------------------------------------------
# batched wrappers: n envs searched at once on one engine (core/batch_search.py)
# ---------------------------------------------------------------------------------------------------
class BatchRoots:
    """Opaque handle of a whole batch: which env (by identity) sits in which slot of the batch's engine and which slots kept a
    re-usable sub-tree.  The caller steps each env with its move and passes the handle back as `root_nodes`."""

    def __init__(self, bs, params, envs, slots, reusable, has_next):
        self._bs, self._params, self._alive = bs, params, True
        self._entries = {id(e): (e, int(s), bool(r), bool(h)) for e, s, r, h in zip(envs, slots, reusable, has_next)}  # (the env object itself: ids are re-used)

    def _entry(self, env):
        ent = self._entries.get(id(env))
        return ent if ent is not None and ent[0] is env else None

    def reusable(self, env):
        """True if `env`'s slot kept a sub-tree for the next search: the chosen child is a node and its position is not terminal."""
        ent = self._entry(env)
        return bool(ent is not None and ent[2])

    def has_next(self, env):
        """True where the reference's search returns a `next_root_node` for `env` (mcts_v2.py:436-446: the chosen move has a child node,
        i.e. it was visited) -- also for the move that ends the game, whose terminal child the engine does not keep (`reusable` is
        False there: a finished env cannot be searched again)."""
        ent = self._entry(env)
        return bool(ent is not None and ent[3])


def _search_many(envs, eval_func, root_nodes, c_puct_base, c_puct_init, num_simulations, num_parallel, root_noise, warm_up, deterministic):
    envs = list(envs)
    for env in envs:
        check_env(env)
    per_env = None  # a sequence: one number of simulations per env; the engine is built at (and the handle remembers) the largest
    if isinstance(num_simulations, (list, tuple, np.ndarray)):
        per_env = slot_simulations(list(num_simulations), len(envs), 1 << 30)
        num_simulations = int(per_env.max()) if len(per_env) else 1
    check_num_simulations(num_simulations)
    if not envs:
        raise ValueError("Expect at least one env")
    if len({id(e) for e in envs}) != len(envs):
        raise ValueError("every env of a batch must be an object of its own")
    for env in envs:
        if env.is_game_over():
            raise RuntimeError("Game is over.")
    if len({env_key(e) for e in envs}) != 1:
        raise ValueError("all envs of a batch must share game, board size, komi / max_steps / num_to_win and num_stack")
    num_stack = getattr(envs[0], "num_stack", 8)
    check_planes(eval_func, 2 * num_stack + 1, num_stack)
    params = (env_key(envs[0]), int(num_simulations), int(num_parallel), float(c_puct_base), float(c_puct_init), bool(root_noise),
              id(getattr(envs[0], "_binding", None)))
    n = len(envs)
    slot_of, keep = [None] * n, []
    if root_nodes is not None:
        if not isinstance(root_nodes, BatchRoots) or not root_nodes._alive or root_nodes._params != params:
            raise ValueError("`root_nodes` must be the handle returned by the previous batched search with the same settings (or None)")
        bs = root_nodes._bs
        if n > bs.capacity:
            raise ValueError(f"{n} envs do not fit the {bs.capacity} slots of this batch; start a larger batch with root_nodes=None")
        out, used = None, set()
        for i, env in enumerate(envs):
            ent = root_nodes._entries.get(id(env))
            if ent is None or ent[0] is not env:
                continue
            slot_of[i] = ent[1]
            used.add(ent[1])
            if ent[2]:  # the slot kept a sub-tree: it must be the tree of the env's position (one export for the whole batch)
                if out is None:
                    out = bs.eng.env_step(None)
                sc = out["scalars"][ent[1]]
                if int(sc[_abi.ENV_TO_PLAY]) != env.to_play or int(sc[_abi.ENV_STEPS]) != env.steps or not np.array_equal(out["board"][ent[1]], env.board):
                    raise ValueError("`root_node` does not belong to this position")
                keep.append(ent[1])
        free = [s for s in range(bs.capacity) if s not in used]
        for i in range(n):  # new envs take free slots; the slots of envs that no longer appear are idled by the load below
            if slot_of[i] is None:
                slot_of[i] = free.pop(0)
        root_nodes._alive, root_nodes._bs = False, None
    else:
        bs = BatchSearch.for_env(envs[0], n, num_simulations, num_parallel, c_puct_base, c_puct_init, root_noise)
        slot_of = list(range(n))
    load = [i for i in range(n) if slot_of[i] not in keep]
    res = bs.load_envs([envs[i] for i in load], slots=[slot_of[i] for i in load], keep=keep)  # LOAD, KEEP and IDLE rows in ONE set_states
    if np.any(res == _abi.SS_GAME_OVER):
        raise RuntimeError("Game is over.")
    if np.any(res != _abi.SS_OK):
        raise ValueError(f"the engine refused the position of env {load[int(np.flatnonzero(res != _abi.SS_OK)[0])]}")
    order = np.argsort(np.asarray(slot_of))  # bs.slots is ascending: row r of the per-slot arrays belongs to env order[r]
    assert np.array_equal(np.asarray(slot_of)[order], bs.slots)
    row_of = np.empty(n, dtype=np.int64)
    row_of[order] = np.arange(n)
    legals = [env.legal_actions for env in envs]
    noise = None
    if root_noise:  # one np.random.dirichlet per env, in list order (add_dirichlet_noise, mcts_v2.py:259-260)
        draws = [np.random.dirichlet(np.ones_like(lg) * 0.03) for lg in legals]
        noise = np.stack([draws[i] for i in order])
    warm = np.broadcast_to(np.asarray(warm_up, dtype=bool), (n,))
    bs.search(eval_func, noise, warm[order], None if per_env is None else per_env[order])
    pis, child_ns, root_qs = bs.results().cpu()
    moves, search_pis = [], []
    for i, env in enumerate(envs):  # the np.random.choice draws of env 0 until its move is acceptable, then env 1, ...
        search_pis.append(pis[row_of[i]])
        moves.append(choose_move(env, search_pis[i], child_ns[row_of[i]], legals[i], warm[i], deterministic))
    child_qs, reusable = bs.commit([int(moves[i]) for i in order])
    handle = BatchRoots(bs, params, envs, slot_of, [reusable[row_of[i]] for i in range(n)],
                        [child_ns[row_of[i]][moves[i]] > 0 for i in range(n)])  # a child node exists iff the move was ever selected
    return (moves, search_pis, [float(root_qs[row_of[i]]) for i in range(n)], [float(child_qs[row_of[i]]) for i in range(n)], handle)


def uct_search_many(envs, eval_func, root_nodes, c_puct_base, c_puct_init, num_simulations=800, root_noise=False, warm_up=False,
                    deterministic=False):
    """`uct_search` for a list of envs at once.  Returns (moves, search_pis, root_Qs, best_child_Qs, next_roots), one entry per env,
    and ONE opaque batch handle `next_roots`: step each env with its move and pass the handle back as `root_nodes`.  The handle maps
    envs (by identity) to slots: envs that no longer appear have their slots idled, new envs take free slots, slots without a
    re-usable sub-tree are loaded again from their env; a slot whose kept tree does not belong to its env's position raises ValueError.
    All envs share game, board size, komi / max_steps / num_to_win and num_stack.  `warm_up` is a bool or one bool per env.
    `num_simulations` is an int, or one int per env: the batch's engine is built at the largest and every env is searched at its own
    number (a later call on the same handle must name the same largest value).

    `eval_func` is called as eval_func(obs, True) with the leaf rows of ALL envs (a batched search needs a batch-capable eval_func);
    an evaluator with `device_eval` on the engine's device runs resident (core/batch_search.py).

    Global NumPy randomness, in this order: before the search one `np.random.dirichlet` per env in list order (when `root_noise`);
    after it the `np.random.choice` draws of env 0 until its move is acceptable, then those of env 1, and so on."""
    return _search_many(envs, eval_func, root_nodes, c_puct_base, c_puct_init, num_simulations, 1, root_noise, warm_up, deterministic)


def parallel_uct_search_many(envs, eval_func, root_nodes, c_puct_base, c_puct_init, num_simulations, num_parallel, root_noise=False,
                             warm_up=False, deterministic=False):
    """`parallel_uct_search` for a list of envs at once; see uct_search_many."""
    return _search_many(envs, eval_func, root_nodes, c_puct_base, c_puct_init, num_simulations, num_parallel, root_noise, warm_up,
                        deterministic)
