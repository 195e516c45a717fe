"""Sample format of the self-play path (reference: alpha_zero/core/replay.py:14-20)."""
from typing import NamedTuple, Optional

import numpy as np


class Transition(NamedTuple):
    state: Optional[np.ndarray]    # int8[2K+1, N, N] observation before the move, mover's perspective (K = num_stack; 17 planes at 8)
    pi_prob: Optional[np.ndarray]  # search policy over all A actions
    value: Optional[float]         # z: +reward for the eventual last player's samples, -reward for the other's


TransitionStructure = Transition(state=None, pi_prob=None, value=None)


class DeviceReplay:
    """UniformReplay (reference alpha_zero/core/replay.py:35-118) with its storage as an HBM ring.

    Same semantics: ring write at `num_samples_added % capacity` (:64-68), `sample` returns None while
    `size < batch_size` and otherwise draws `random_state.randint(0, size, batch_size)` with replacement (:72-83), so with
    the same RandomState and the same games the batches equal the reference's.  What is different is where the data
    lives: harvested games go from the engine's output tensors into the ring device-to-device (`add_harvest`), and
    `sample_device` returns the batch as device tensors, already transformed by one dihedral op and cast for the network
    (core/pipeline.py:636-643), from one gather kernel (`azsp_replay_gather`) -- no host round trip per batch.
    `add_game` / `sample` / `get_state` / `set_state` keep the reference's host-side signatures.
    aux_targets=True (no counterpart in the reference: opt-in) adds three rings for the auxiliary targets of `Engine.harvest(with_aux=True)`
    -- ownership int8[capacity, N, N], score and root_q float32[capacity] -- written with the samples (`aux=`) and gathered by
    `sample_device(with_aux=True)` in the same launch, the ownership under the same dihedral op as the state planes.
    `add_samples(weights=)` / `add_harvest(weights=)` (policy surprise weighting, no counterpart in the reference: opt-in) write every row as
    often as its weight says (`azsp_replay_add_weighted`); the ring then holds plain rows, and every read is what it was."""

    def __init__(self, capacity, random_state, board_size, num_actions, channels=17, device="cuda", binding=None, pi_dtype=np.float64,
                 aux_targets=False):
        import torch

        if capacity <= 0:
            raise ValueError(f"Expect capacity to be a positive integer, got {capacity}")
        if binding is None:
            from .. import _lib

            binding = _lib.load(require_gpu=True)
        self.b = binding
        self.structure = TransitionStructure
        self.capacity, self.random_state = capacity, random_state
        self.N, self.A, self.C = board_size, num_actions, channels
        self.device = torch.device(device)
        self.pi_dtype = pi_dtype
        self.states = torch.zeros((capacity, channels, board_size, board_size), dtype=torch.int8, device=self.device)
        self.pi = torch.zeros((capacity, num_actions), dtype=torch.float32, device=self.device)
        self.z = torch.zeros((capacity,), dtype=torch.float32, device=self.device)
        self.aux_targets = bool(aux_targets)
        if self.aux_targets:
            self.ownership = torch.zeros((capacity, board_size, board_size), dtype=torch.int8, device=self.device)
            self.score = torch.zeros((capacity,), dtype=torch.float32, device=self.device)
            self.root_q = torch.zeros((capacity,), dtype=torch.float32, device=self.device)
        self.num_games_added = 0
        self.num_samples_added = 0

    # -- writes ------------------------------------------------------------------------------------------------------
    def _check_aux(self, aux, n):
        """`aux` as the writes take it: (ownership, score, root_q) with one row per sample, required exactly when the replay has the rings."""
        if self.aux_targets != (aux is not None):
            raise ValueError("aux=(ownership, score, root_q) is required by a replay built with aux_targets=True and refused by one without")
        if aux is not None and (len(aux) != 3 or any(int(t.shape[0]) != n for t in aux)):
            raise ValueError(f"`aux` must be (ownership, score, root_q) with one row per sample ({n})")

    def _add_weighted(self, states, pi, z, aux, weights):
        """Row i is appended c_i = floor(w_i) + (u_i < w_i - floor(w_i)) times, u = random_state.random_sample(n): one uniform per row,
        rows with integer weights included.  One count-and-scan launch and one scatter launch (azsp_replay_add_weighted); the host reads
        the total (4 bytes) to advance num_samples_added."""
        import ctypes

        import torch

        n = int(z.shape[0])
        w = torch.as_tensor(weights).to(self.device, torch.float32).reshape(-1).contiguous()
        if w.shape[0] != n:
            raise ValueError(f"`weights` must hold one weight per sample ({n}), got {w.shape[0]}")
        u = torch.from_numpy(np.asarray(self.random_state.random_sample(n), dtype=np.float64)).to(self.device)
        if n == 0:
            return
        states = torch.as_tensor(states).to(self.device, torch.int8).reshape((n,) + self.states.shape[1:]).contiguous()
        pi = torch.as_tensor(pi).to(self.device, torch.float32).reshape(n, self.A).contiguous()
        z = torch.as_tensor(z).to(self.device, torch.float32).reshape(n).contiguous()
        rings = (self.ownership, self.score, self.root_q) if aux is not None else ()
        srcs = [torch.as_tensor(t).to(self.device, ring.dtype).reshape((n,) + ring.shape[1:]).contiguous() for ring, t in zip(rings, aux or ())]
        ofs = torch.empty((n + 1,), dtype=torch.int32, device=self.device)
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream) if self.device.type == "cuda" else None
        rc = self.b.dll.azsp_replay_add_weighted(self.states.data_ptr(), self.pi.data_ptr(), self.z.data_ptr(), self.capacity, self.num_samples_added,
                                                 states.data_ptr(), pi.data_ptr(), z.data_ptr(), n, self.C, self.N, self.A, w.data_ptr(), u.data_ptr(),
                                                 *([t.data_ptr() for t in rings] or [None] * 3), *([t.data_ptr() for t in srcs] or [None] * 3),
                                                 ofs.data_ptr(), stream)
        if rc != 0:
            raise RuntimeError(f"azsp_replay_add_weighted failed with code {rc}")
        self.num_samples_added += int(ofs[n])  # (synchronises: the sources may be re-used once this returns)

    def add_samples(self, states, pi, z, num_games=1, aux=None, weights=None):
        """Appends samples in order (device or host tensors): the ring positions the reference's per-transition loop
        would have written (:55-68).  More samples than the capacity keep only the last `capacity` (the earlier ones
        would have been overwritten by the same call).  aux: (ownership, score, root_q) of the same rows, with aux_targets.
        weights: an optional float per sample (e.g. the actor's `last_harvest_weight`): the row is written floor(w) times and once more
        with probability w - floor(w) (a NaN or negative weight: never), as if the rows had been repeated that often and then appended."""
        import torch

        n = int(z.shape[0])
        self._check_aux(aux, n)
        if weights is not None:
            self._add_weighted(states, pi, z, aux, weights)
            self.num_games_added += num_games
            return
        if n:
            states = torch.as_tensor(states).to(self.device, torch.int8)
            pi = torch.as_tensor(pi).to(self.device, torch.float32)
            z = torch.as_tensor(z).to(self.device, torch.float32)
            skip = max(0, n - self.capacity)
            pos = (torch.arange(self.num_samples_added + skip, self.num_samples_added + n, device=self.device, dtype=torch.int64)
                   % self.capacity)
            self.states.index_copy_(0, pos, states[skip:])
            self.pi.index_copy_(0, pos, pi[skip:])
            self.z.index_copy_(0, pos, z[skip:])
            if aux is not None:
                for ring, t in zip((self.ownership, self.score, self.root_q), aux):
                    ring.index_copy_(0, pos, torch.as_tensor(t).to(self.device, ring.dtype).reshape((n,) + ring.shape[1:])[skip:])
            self.num_samples_added += n
        self.num_games_added += num_games

    def add_harvest(self, states, pi, z, games, keep=None, aux=None, weights=None):
        """Everything `SelfPlayActor.harvest_tensors()` returned: finished games, concatenated in harvest order.  keep: an optional
        bool per sample (e.g. the actor's `last_harvest_full` under a playout cap): only those rows are stored, in order; the games
        count as before.  aux: the actor's `last_harvest_aux` of the same harvest (with aux_targets), filtered by `keep` like the samples.
        weights: the actor's `last_harvest_weight` of the same harvest (policy surprise weighting) instead of `keep` (both: ValueError):
        every row is stored as often as its weight says, `add_samples(weights=)`; a fast move has weight 0 unless it earned a share."""
        if weights is not None and keep is not None:
            raise ValueError("`weights` and `keep` cannot be given together: a weight of 0 drops a row")
        self._check_aux(aux, int(z.shape[0]))
        if keep is not None:
            import torch

            k = torch.as_tensor(keep).to(torch.bool).reshape(-1)
            if k.shape[0] != int(z.shape[0]):
                raise ValueError(f"`keep` must hold one flag per sample ({int(z.shape[0])}), got {k.shape[0]}")
            states, pi, z = (torch.as_tensor(t)[k.to(torch.as_tensor(t).device)] for t in (states, pi, z))
            if aux is not None:
                aux = tuple(torch.as_tensor(t)[k.to(torch.as_tensor(t).device)] for t in aux)
        self.add_samples(states, pi, z, num_games=len(games), aux=aux, weights=weights)

    def add_game(self, game_seq):
        import torch

        if len(game_seq) == 0:
            self.num_games_added += 1
            return
        self.add_samples(torch.from_numpy(np.stack([t.state for t in game_seq])), torch.from_numpy(np.stack([t.pi_prob for t in game_seq]).astype(np.float32)),
                         torch.tensor([float(t.value) for t in game_seq], dtype=torch.float32))

    @property
    def size(self):
        return min(self.num_samples_added, self.capacity)

    # -- reads -------------------------------------------------------------------------------------------------------
    def _gather(self, indices, op, state_dtype, with_aux=False):
        import ctypes

        import torch

        from .. import _abi

        code = {torch.int8: _abi.FEAT_I8, torch.float32: _abi.FEAT_F32, torch.bfloat16: _abi.FEAT_BF16, torch.float16: _abi.FEAT_F16}[state_dtype]
        B = len(indices)
        idx = torch.as_tensor(np.asarray(indices, dtype=np.int64)).to(self.device)
        st = torch.empty((B, self.C, self.N, self.N), dtype=state_dtype, device=self.device)
        pi = torch.empty((B, self.A), dtype=torch.float32, device=self.device)
        z = torch.empty((B,), dtype=torch.float32, device=self.device)
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream) if self.device.type == "cuda" else None
        if with_aux:  # the same launch gathers the auxiliary rings, the ownership under the same op
            own = torch.empty((B, self.N, self.N), dtype=torch.float32, device=self.device)
            sc = torch.empty((B,), dtype=torch.float32, device=self.device)
            rq = torch.empty((B,), dtype=torch.float32, device=self.device)
            rc = self.b.dll.azsp_replay_gather_aux(self.states.data_ptr(), self.pi.data_ptr(), self.z.data_ptr(), idx.data_ptr(), B, self.C, self.N,
                                                   self.A, int(op), code, st.data_ptr(), pi.data_ptr(), z.data_ptr(), self.ownership.data_ptr(),
                                                   self.score.data_ptr(), self.root_q.data_ptr(), own.data_ptr(), sc.data_ptr(), rq.data_ptr(), stream)
            if rc != 0:
                raise RuntimeError(f"azsp_replay_gather_aux failed with code {rc}")
            return st, pi, z, own, sc, rq
        rc = self.b.dll.azsp_replay_gather(self.states.data_ptr(), self.pi.data_ptr(), self.z.data_ptr(), idx.data_ptr(), B, self.C, self.N, self.A,
                                           int(op), code, st.data_ptr(), pi.data_ptr(), z.data_ptr(), stream)
        if rc != 0:
            raise RuntimeError(f"azsp_replay_gather failed with code {rc}")
        return st, pi, z

    def sample(self, batch_size):
        """Reference signature (:72-83): Transition of stacked numpy arrays, or None while the replay is too small."""
        if self.size < batch_size:
            return None
        indices = self.random_state.randint(low=0, high=self.size, size=batch_size)
        st, pi, z = self._gather(indices, 0, __import__("torch").int8)
        return Transition(st.cpu().numpy(), pi.cpu().numpy().astype(self.pi_dtype), z.cpu().numpy().astype(np.float64))

    def sample_device(self, batch_size, transform=None, state_dtype=None, with_aux=False):
        """The batch as device tensors (states cast to `state_dtype`, default float32 like core/pipeline.py:636).
        transform: None, an op code 0..7 (azsp_dihedral numbering) or "random" = apply_random_transformation
        (utils/transformation.py:160-167: with probability 0.5 one of the five reference transforms for the whole batch,
        chosen with Python's `random`).  with_aux=True (a replay built with aux_targets) returns (states, pi, z, ownership float32[B,N,N],
        score float32[B], root_q float32[B]): the ownership under the same op as the states, score and root_q as stored."""
        import random

        import torch

        if with_aux and not self.aux_targets:
            raise ValueError("with_aux=True needs a replay built with aux_targets=True")
        if self.size < batch_size:
            return None
        indices = self.random_state.randint(low=0, high=self.size, size=batch_size)
        op = 0
        if transform == "random":
            if random.random() > 0.5:
                op = {"h_flip": 1, "v_flip": 2, "rotate90": 3, "rotate180": 4, "rotate270": 5}[random.choice(["h_flip", "v_flip", "rotate90", "rotate180", "rotate270"])]
        elif transform is not None:
            op = int(transform)
        return self._gather(indices, op, state_dtype or torch.float32, with_aux)

    # -- persistence (reference dictionary, :99-111; uncompressed transitions) ----------------------------------------
    def get_state(self):
        n = self.size
        st, pi, z = self.states[:n].cpu().numpy(), self.pi[:n].cpu().numpy().astype(self.pi_dtype), self.z[:n].cpu().numpy()
        storage = [Transition(st[i].copy(), pi[i].copy(), float(z[i])) for i in range(n)] + [None] * (self.capacity - n)
        out = {"num_games_added": self.num_games_added, "num_samples_added": self.num_samples_added, "storage": storage}
        if self.aux_targets:  # next to the reference's keys, which stay as they are: the first `size` rows of the three rings
            out["aux"] = {"ownership": self.ownership[:n].cpu().numpy(), "score": self.score[:n].cpu().numpy(), "root_q": self.root_q[:n].cpu().numpy()}
        return out

    def set_state(self, state):
        import torch

        storage = state["storage"]
        for i, t in enumerate(storage[: self.capacity]):
            if t is None:
                continue
            s = t.state
            if isinstance(s, tuple):  # the reference's snappy-compressed form (compress_array, :24-26)
                import snappy

                s = np.frombuffer(snappy.uncompress(s[0]), dtype=s[2]).reshape(s[1])
            self.states[i] = torch.from_numpy(np.ascontiguousarray(s)).to(self.device)
            self.pi[i] = torch.from_numpy(np.asarray(t.pi_prob, dtype=np.float32)).to(self.device)
            self.z[i] = float(t.value)
        if self.aux_targets:  # a state without the key (a reference replay, or one saved without aux targets) loads with zero rings
            aux = state.get("aux")
            for ring, key in ((self.ownership, "ownership"), (self.score, "score"), (self.root_q, "root_q")):
                ring.zero_()
                if aux is not None:
                    rows = torch.from_numpy(np.ascontiguousarray(aux[key]))[: self.capacity]
                    ring[: rows.shape[0]] = rows.to(self.device, ring.dtype)
        self.num_games_added = state["num_games_added"]
        self.num_samples_added = state["num_samples_added"]
