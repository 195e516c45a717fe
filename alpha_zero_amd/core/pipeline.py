"""Self-play actor on the batched engine (reference: alpha_zero/core/pipeline.py:83-382).

`game_stats_from_row` rebuilds the per-game `stats` dict of play_and_record_one_game
(pipeline.py:367-380) from the game row (include/azsp.h AZSP_GR_*, mirrored as _abi.GR_*) the engine emits at harvest time.
"""
from typing import Any, Dict, NamedTuple

import numpy as np

from .. import _abi


def _result_string(row, game, komi):
    """go.py:194-200 + go_engine.py:527-534 / gomoku.py:138-147"""
    winner = int(row[_abi.GR_WINNER])
    if game == "go":
        if int(row[_abi.GR_RESIGNED]):
            return "B+R" if winner == 1 else "W+R"
        score = float(int(row[_abi.GR_AREA_BLACK])) - (float(int(row[_abi.GR_AREA_WHITE])) + komi)
        if score > 0:
            return "B+" + "%.1f" % score
        if score < 0:
            return "W+" + "%.1f" % abs(score)
        return "DRAW"
    return "B+1.0" if winner == 1 else "W+1.0" if winner == 2 else "DRAW"


def game_stats_from_row(row, game: str, komi: float = 7.5, resign_threshold: float = -1.0) -> Dict[str, Any]:
    """`row`: one game row int32[GR_COUNT] of Engine.harvest() (azsp_harvest's games_host)."""
    stats: Dict[str, Any] = {"game_length": int(row[_abi.GR_LENGTH]), "game_result": _result_string(row, game, komi)}
    if game == "go":  # has_pass_move / has_resign_move (pipeline.py:372-380)
        stats["num_passes"] = int(row[_abi.GR_PASSES])
        stats["is_resign_disabled"] = bool(row[_abi.GR_RESIGN_DISABLED])
        stats["is_marked_for_resign"] = bool(row[_abi.GR_MARKED])
        stats["is_could_won"] = bool(row[_abi.GR_COULD_WON])
        mp = int(row[_abi.GR_MARKED_PLAYER])
        stats["marked_resign_player"] = "B" if mp == 1 else "W" if mp == -1 else None
        stats["resign_threshold"] = resign_threshold
    return stats


# =====================================================================================================
# Batched self-play actor
# =====================================================================================================
import time  # noqa: E402
import warnings  # noqa: E402

import torch  # noqa: E402

from .engine import Engine, EngineConfig, SearchOptions, check_num_stack, policy_surprise_params, visit_reduction_params  # noqa: E402
from .network import AlphaZeroNet, InferenceNet, capture_graph, widen_for_kernels  # noqa: E402
from .replay import Transition  # noqa: E402

def check_input_channels(network, num_stack):
    """The engine's observations have 2 * num_stack + 1 planes (base.py:228-266); a network whose stem takes another count is refused
    here instead of inside a kernel."""
    cin = network.conv_block[0].in_channels
    if cin != 2 * num_stack + 1:
        raise ValueError(f"the network's stem takes {cin} input planes, but num_stack = {num_stack} observations have {2 * num_stack + 1}")


_FEAT_OF = {torch.float32: _abi.FEAT_F32, torch.bfloat16: _abi.FEAT_BF16, torch.float16: _abi.FEAT_F16}


class ClampWindow:
    """Which games may hold a move that was searched on a CLAMPING fp32-class evaluator (Weak #1).  The range record says
    that some kernel lane clamped since the last poll, not which board: every game that ran a round inside the window
    (last clean poll, detecting poll] is suspect -- the games in progress at the detecting poll and the finished games not handed out
    yet.  The reference's fp32 forward (pipeline.py:102-109) has no such window, so none of their samples may reach the learner
    unmarked.  Games are identified by the engine's uid = (games finished before in that slot) * G + slot."""

    _NONE_LO, _NONE_HI = np.iinfo(np.int64).max, -1

    def __init__(self, num_games):
        self.G = int(num_games)
        self.next_unharvested = np.zeros(self.G, dtype=np.int64)  # per slot: first game index no harvest has handed out yet
        self.lo = np.full(self.G, self._NONE_LO, dtype=np.int64)   # per slot: suspect game indices [lo, hi]
        self.hi = np.full(self.G, self._NONE_HI, dtype=np.int64)
        self.events = 0

    def on_event(self, games_done):
        """games_done int[G]: azsp_get_status column 5 at the detecting poll (= the index of each slot's game in progress)."""
        gd = np.asarray(games_done, dtype=np.int64).reshape(self.G)
        self.lo = np.minimum(self.lo, self.next_unharvested)
        self.hi = np.maximum(self.hi, gd)
        self.events += 1

    def mask(self, uids):
        """bool per harvested game (uids = column 11 of the harvest rows): suspect?  Advances the per-slot harvest front."""
        u = np.asarray(uids, dtype=np.int64)
        slot, idx = u % self.G, u // self.G
        m = (idx >= self.lo[slot]) & (idx <= self.hi[slot])
        np.maximum.at(self.next_unharvested, slot, idx + 1)
        spent = self.next_unharvested > self.hi  # intervals wholly behind the harvest front are used up
        self.lo[spent], self.hi[spent] = self._NONE_LO, self._NONE_HI
        return m


class HarvestAux(NamedTuple):
    """The auxiliary targets of one harvest (SelfPlayActor.last_harvest_aux), row for row with its states: Engine.harvest(with_aux=True)."""
    ownership: torch.Tensor  # int8[n, N, N]  +1 the mover's point, -1 the opponent's, 0 nobody's, in the game's final position
    score: torch.Tensor      # float32[n]     Go: final area score with komi, seen by the mover; Gomoku: z
    root_q: torch.Tensor     # float32[n]     root value of the sample's search


class SelfPlayActor:
    """G concurrent self-play games on one GPU: replaces G `run_selfplay_actor_loop` processes
    (pipeline.py:166-286).  One round = engine kernel (expand/backup of the previous leaf batch, end-of-move
    work, selection of the next P leaves per game, observation planes) + one network forward on G*P rows.
    Nothing returns to the host during a round; finished games are collected with `harvest()`."""

    def __init__(self, network: AlphaZeroNet, *, game="go", board_size=9, num_games=4096, num_simulations=200, num_parallel=8,
                 c_puct_base=19652.0, c_puct_init=1.25, warm_up_steps=16, check_resign_after_steps=40, disable_resign_ratio=0.1,
                 resign_threshold=-1.0, komi=7.5, num_to_win=5, seed=1, rank=0, device="cuda", net_dtype=torch.float32,
                 use_graph=True, training_steps=0, binding=None, root_noise=True, deterministic=False, tiled_features=None, engine_kw=None,
                 use_split_evaluator=True, auto_widen=None, num_stack=8, split_any_board=False, playout_cap=None,
                 leaf_symmetry=None, forced_playouts=None, prune_policy_target=True, gumbel=None, aux_targets=False,
                 policy_surprise=None, fpu_reduction=None, visit_reduction=None):
        """net_dtype: precision class of the leaf evaluator.  The default is the REFERENCE'S: fp32 (pipeline.py:91-123 evaluates in fp32,
        no autocast anywhere) -- on the hand-written split-precision kernels (hi + lo f16 pairs, three MFMA products, fp32 accumulation:
        include/azsp.h azsp_conv3x3_split) for 9x9 x {128, 64} and 13x13 Gomoku x 64 networks, on library fp32 convolutions (announced
        by a RuntimeWarning) for any other shape.  torch.bfloat16 / torch.float16 are the opt-in lower-precision evaluators.
        tiled_features: None = the engine writes its observation planes in the evaluator's own input layout whenever the network / board
        shape has hand-written kernels (tiled bf16 / f16, or the fp32-class stem's split layout); False = always NCHW planes.
        use_split_evaluator: False = an fp32 network is evaluated by the LIBRARY's fp32 convolutions even where the split-precision
        kernels exist (comparison runs: bench.py's fp32_library_companion, tests/test_precision_parity.py).
        split_any_board: True = InferenceNet.use_split_any_board on every evaluator this actor builds: an fp32 network on a board without a
        tailored stem (19x19 / 13x13 Go, 15x15 Gomoku, 256 filters) runs stem, tower and heads on the hand-written kernels and the engine
        writes AZSP_FEAT_F16_SPLIT, instead of the split tower behind a library stem and heads.  Off by default.
        auto_widen: networks of a width without hand-written kernels run as a function-preserving widened copy (network.widen_for_kernels).
        None = on the GPU whenever the widened network actually reaches hand-written kernels (not for library comparison runs, not when
        the caller disabled the kernels' feature layouts); True / False force it.
        num_stack: history boards per observation (the env's num_stack, 1..8): the engine writes 2 * num_stack + 1 planes, which must be
        the network's input channels.
        playout_cap, leaf_symmetry, forced_playouts, prune_policy_target, gumbel, fpu_reduction: the opt-in search rules, SearchOptions.of.  Under a
        playout cap every move is recorded; `harvest()` hands the learner the full-search samples only, `harvest_tensors()` leaves the
        flags in `last_harvest_full`.
        aux_targets: True = every sample carries the auxiliary training targets (Engine.set_aux_targets: ownership of the final position,
        final score, root value of its search, all in the mover's perspective); `harvest_tensors()` leaves them in `last_harvest_aux`.
        Off by default; not with a drop-in engine (engine_kw stop_after_move: ValueError), which records no samples.
        policy_surprise: None, frac or (frac, include_fast) (Engine.set_policy_surprise): every sample carries the KL divergence of its
        policy target from its root's raw prior and the weight that follows from it; `harvest_tensors()` leaves them in
        `last_harvest_surprise` / `last_harvest_weight`, and `DeviceReplay.add_harvest(weights=actor.last_harvest_weight)` writes every
        row as often as its weight says -- with include_fast also the fast moves of a playout cap that `keep=last_harvest_full` drops.
        Off by default; not with a drop-in engine (ValueError).
        visit_reduction: None or (threshold, lookback, min_simulations, min_weight) (Engine.set_visit_reduction): once one side has led
        by more than `threshold` in the last `lookback` searches of a game, its moves are searched with fewer simulations and their
        samples carry a base weight below 1; `harvest_tensors()` leaves the bases in `last_harvest_base` beside `last_harvest_full` and
        the weights (base * full, or with policy_surprise the surprise weights with the base in them) in `last_harvest_weight`.  Off
        by default; not with a drop-in engine (ValueError).  The reference-format `harvest()` has no weight column and ignores it."""
        opt = SearchOptions.of(leaf_symmetry, forced_playouts, prune_policy_target, gumbel, playout_cap, num_simulations,
                               fpu_reduction)  # ValueError before anything is built
        from .. import _lib

        self.leaf_symmetry, self.forced_playouts, self.prune_policy_target = opt.leaf_symmetry, opt.forced_k, opt.prune_policy_target
        self.gumbel, self.playout_cap = opt.gumbel if gumbel is not None else None, opt.playout_cap
        self.fpu_reduction = opt.fpu[1:] if opt.fpu[0] else None
        self.num_stack = check_num_stack(num_stack)
        check_input_channels(network, self.num_stack)

        self.binding = binding or _lib.load(require_gpu=True)
        self.device = torch.device(device)
        self.game, self.komi, self.resign_threshold = game, komi, resign_threshold
        self.net_dtype = net_dtype
        self.use_graph = use_graph and self.device.type == "cuda"
        self.use_split_evaluator = bool(use_split_evaluator)
        self.split_any_board = bool(split_any_board)
        if auto_widen is None:  # widening only pays when the wider network lands on hand-written kernels
            auto_widen = (self.device.type == "cuda" and tiled_features is not False
                          and (net_dtype != torch.float32 or self.use_split_evaluator))
        self.auto_widen = bool(auto_widen)
        self.board_size = board_size
        wnet, self._widen_note = widen_for_kernels(network, board_size, net_dtype) if self.auto_widen else (network, "")
        self.infer = self._inference_net(wnet)  # decides the engine's feature layout; moved to the device as the first evaluator below
        self.tiled_features = self.infer.supports_tiled_features(board_size, self.device) if tiled_features is None else bool(tiled_features)
        # fp32-class evaluator: the engine writes the stem's input layout itself (AZSP_FEAT_F16_SPLIT; 0 / 1 planes are exact f16 values)
        self.split_features = tiled_features is None and not self.tiled_features and self.infer.supports_split_features(board_size, self.device)
        self._library_stem = tiled_features is not None and not self.tiled_features  # (NCHW planes although the tiled kernels exist)
        if self.device.type == "cuda" and "hand-written" not in self.evaluator_path:
            warnings.warn(f"alpha_zero_amd: evaluator falls back to {self.evaluator_path}", RuntimeWarning, stacklevel=2)
        self.cfg = EngineConfig(
            game=game, board_size=board_size, num_games=num_games, num_parallel=num_parallel, num_simulations=num_simulations,
            c_puct_base=c_puct_base, c_puct_init=c_puct_init, warm_up_steps=warm_up_steps, komi=komi, num_to_win=num_to_win,
            resign_threshold=resign_threshold, check_resign_after_steps=check_resign_after_steps,
            disable_resign_ratio=disable_resign_ratio, root_noise=root_noise, deterministic=deterministic,
            feature_dtype=((_abi.FEAT_F16_TILED if net_dtype == torch.float16 else _abi.FEAT_BF16_TILED) if self.tiled_features
                           else _abi.FEAT_F16_SPLIT if self.split_features else _FEAT_OF[net_dtype]),
            training_steps=training_steps, seed=seed, rank=rank, num_stack=self.num_stack,
            device_index=self.device.index or 0, leaf_symmetry=leaf_symmetry,  # (set before the first root is selected)
            forced_playouts=forced_playouts, gumbel=gumbel, fpu_reduction=fpu_reduction)
        for k, v in (engine_kw or {}).items():  # further EngineConfig fields (move logs, max_plies, ...: tests and diagnostics)
            if not hasattr(self.cfg, k):
                raise TypeError(f"unknown engine option {k}")
            setattr(self.cfg, k, v)
        self.aux_targets = bool(aux_targets) or bool(self.cfg.aux_targets)
        if self.aux_targets and self.cfg.stop_after_move:
            raise ValueError("aux_targets needs the batched actor: a drop-in engine (stop_after_move) records no samples")
        self.cfg.aux_targets = self.aux_targets
        if policy_surprise is not None:
            self.cfg.policy_surprise = policy_surprise
        self.policy_surprise = policy_surprise_params(self.cfg.policy_surprise)[0] != 0  # (ValueError for a malformed value, before the engine is built)
        if self.policy_surprise and self.cfg.stop_after_move:
            raise ValueError("policy_surprise needs the batched actor: a drop-in engine (stop_after_move) records no samples")
        if visit_reduction is not None:
            self.cfg.visit_reduction = visit_reduction
        self.visit_reduction = visit_reduction_params(self.cfg.visit_reduction, num_simulations)[0] != 0  # (ValueError for a malformed value, before the engine is built)
        if self.visit_reduction and self.cfg.stop_after_move:
            raise ValueError("visit_reduction needs the batched actor: a drop-in engine (stop_after_move) plays no games")
        self.engine = Engine(self.binding, self.cfg, device=self.device, prune_policy_target=self.prune_policy_target, playout_cap=self.playout_cap)
        self.last_harvest_full = torch.zeros(0, dtype=torch.bool, device=self.device)
        self.last_harvest_aux = None  # HarvestAux of the last harvest_tensors() (aux_targets=True only)
        self.last_harvest_surprise = self.last_harvest_weight = None  # float32[n] of the last harvest_tensors() (policy_surprise only; the weight with visit_reduction too)
        self.last_harvest_base = None  # float32[n] of the last harvest_tensors() (visit_reduction only)
        self.engine.reset_games()
        self._graph = None
        self.rounds = 0
        self.straddled_games = 0  # harvested games that were in progress across a weight hot-swap (see harvest())
        # fp32-class evaluator: clamped out-of-range activations seen so far and the rescalings they triggered (_check_evaluator_range)
        self.range_events, self.range_max_abs, self.range_rescales = 0, 0.0, 0
        # games that ran a round between a clamp event and its repair (ClampWindow): harvest() marks them `evaluator_clamped` or, with
        # drop_clamped_games = True (run_selfplay_actor_loop), drops them; harvest_tensors() leaves a bool per game in last_harvest_clamped
        self.clamp_window = ClampWindow(num_games)
        self.drop_clamped_games, self.clamped_games, self.last_harvest_clamped = False, 0, np.zeros(0, dtype=bool)
        self.drop_straddling_games = False
        self._install(self.infer, training_steps)

    # -- weights ---------------------------------------------------------------------------------------
    def _inference_net(self, network):
        """The evaluator of `network`, still on the host (what it supports on self.device does not depend on where it lives)."""
        inf = InferenceNet(network, dtype=self.net_dtype, binding=self.binding if self.device.type == "cuda" else None)
        inf.use_split_tower = self.use_split_evaluator
        inf.use_split_any_board = self.split_any_board
        return inf

    def _install(self, infer, training_steps):
        self.infer, self.training_steps, self._graph = infer.to(self.device), training_steps, None
        self.engine.set_actor_state(self.resign_threshold, training_steps)  # games that start from now on carry this tag

    def set_network(self, network: AlphaZeroNet, training_steps=0):
        """Checkpoint hot-swap (pipeline.py:232-239): new weights take effect at the next round."""
        check_input_channels(network, self.num_stack)
        if self.auto_widen:
            network, _ = widen_for_kernels(network, self.board_size, self.net_dtype)
        self._install(self._inference_net(network), training_steps)

    @property
    def evaluator_path(self):
        """Which kernels this actor's forward runs on, derived from the live InferenceNet: its evaluator_path (or the library stem the
        caller asked for), the widen note, and the activation shift its calibration chose (a hot-swapped network starts without one)."""
        inf = self.infer
        base = "library stem (tiled features disabled by the caller)" if self._library_stem else inf.evaluator_path(self.board_size, self.device)
        shift = (f"; activations carried x 2^-{inf.act_shift} (exact rescaling, calibrated max |v| = {inf.act_max_abs:.4g})"
                 if self.split_features and inf.act_shift and not inf.split_fallback_reason else "")
        return base + self._widen_note + shift

    def set_resign_threshold(self, resign_threshold):
        """var_resign_threshold as the reference actor reads it before EVERY game (pipeline.py:241-242): games that start after this
        call use (and report) the new value, games in progress keep theirs.  <= -1 disables resignation (pipeline.py:449-459)."""
        self.resign_threshold = float(resign_threshold)
        self.engine.set_actor_state(self.resign_threshold, self.training_steps)

    def _forward(self):
        """The forward on the leaf rows the engine has just written, in scratch slot 0 (this actor's own: InferenceNet._scratch)."""
        e = self.engine
        self.infer.forward_rows(e.features, "tiled" if e.features_tiled else "split" if e.features_split else "planes", e.rows, e.N,
                                e.priors, e.values, slot=0)

    def _calibrate(self):
        """fp32-class evaluator: one calibration pass on the leaf batch the engine has just written (InferenceNet.calibrate_activation_scale)
        fixes the power-of-two activation scale of this network BEFORE its first forward is used (and before a hipGraph is captured)."""
        e, inf = self.engine, self.infer
        if e.features_split and inf.supports_split_features(e.N, self.device):
            inf.calibrate_activation_scale(e.features, split_features=(e.rows, e.N), slot=0)
            self._announce_fallback()

    def _announce_fallback(self):
        if self.infer.split_fallback_reason:  # the calibration gave the fp32-class kernels up for this network
            warnings.warn(f"alpha_zero_amd: evaluator falls back to {self.evaluator_path}", RuntimeWarning, stacklevel=3)
            self._graph = None

    # -- rounds ----------------------------------------------------------------------------------------
    def run_round(self, evs=None):
        """evs: optional 4 torch.cuda.Events recorded around (expand/backup + end-of-move), select, forward."""
        e = self.engine
        if evs is not None:
            evs[0].record()
        e.expand_backup()
        if evs is not None:
            evs[1].record()
        e.select()
        if evs is not None:
            evs[2].record()
        if not self.infer.act_calibrated:
            self._calibrate()
        if self.use_graph:
            if self._graph is None:
                self._graph = capture_graph(self._forward, self.device, 3)  # (3 warm-ups: the library picks its kernels before the capture)
            self._graph.replay()
        else:
            self._forward()
        if evs is not None:
            evs[3].record()
        self.rounds += 1

    def run_rounds(self, n):
        for _ in range(n):
            self.run_round()

    # -- output ----------------------------------------------------------------------------------------
    def harvest_tensors(self, clone=False):
        """(states, pi, z, games) of the finished games as device tensors.  The tensors are views of buffers the engine re-uses: the
        next harvest overwrites them in place.  clone=True returns private copies (for consumers that keep them across harvests,
        e.g. an asynchronous learner or a replay insert on another stream).  With aux_targets the auxiliary targets of the same rows
        are left in `last_harvest_aux` (ownership int8[n,N,N], score float32[n], root_q float32[n]; views or clones like the rest).
        With policy_surprise the surprise and the weight of the same rows are left in `last_harvest_surprise` / `last_harvest_weight`
        (float32[n] each; views or clones like the rest).  With visit_reduction the base weights are left in `last_harvest_base` and the
        weights, which then carry the base, in `last_harvest_weight`."""
        got = self.engine.harvest(with_class=True, with_aux=self.aux_targets, with_surprise=self.policy_surprise, with_base=self.visit_reduction)
        st, pi, z, games, full = got[:5]
        if self.aux_targets:
            self.last_harvest_aux = HarvestAux(*(t.clone() if clone else t for t in got[5:8]))
        if self.policy_surprise:
            at = 8 if self.aux_targets else 5
            self.last_harvest_surprise, self.last_harvest_weight = (t.clone() if clone else t for t in got[at:at + 2])
        if self.visit_reduction:
            self.last_harvest_base = got[-2].clone() if clone else got[-2]
            if not self.policy_surprise:
                self.last_harvest_weight = got[-1].clone() if clone else got[-1]
        self._check_evaluator_range()
        self.last_harvest_clamped = self.clamp_window.mask(games[:, _abi.GR_UID]) if len(games) else np.zeros(0, dtype=bool)
        self.clamped_games += int(self.last_harvest_clamped.sum())
        self.last_harvest_full = full != 0  # bool per sample (a new tensor): False = a fast move of the playout cap, not for the learner
        return (st.clone(), pi.clone(), z.clone(), games) if clone else (st, pi, z, games)

    def poll_evaluator_range(self):
        """Poll the fp32-class evaluator's range record now (two words; synchronises the stream) instead of waiting for the next
        harvest: an event is repaired at once and the games that ran inside the window are remembered (ClampWindow).  The actor loop
        calls this every few rounds, which bounds the window by that many rounds.  Returns the events seen so far."""
        self._check_evaluator_range()
        return self.range_events

    def _check_evaluator_range(self):
        """fp32-class evaluator: its kernels carry values as f16 pairs and clamp what exceeds +-65504 (in units of 2^act_shift) -- the
        reference's fp32 network would carry such a value on.  The kernels record every such event in THIS network's range record
        (InferenceNet.range_rec; another actor or evaluator in the same process has its own); it is polled here, once per harvest (the
        harvest has synchronised the stream already).  An event is counted, announced and ACTED on: the network is re-calibrated on
        the current leaf batch (a larger exact power-of-two activation scale), or, if the format cannot carry it, handed to the
        library's fp32 convolutions -- the actor never keeps playing on a clamping evaluator PAST THE POLL; what ran
        between the event and the poll is marked (ClampWindow: harvest() marks or drops those games)."""
        inf, e = self.infer, self.engine
        ev, mx = inf.read_range()
        if not ev:
            return
        self.range_events += ev
        self.range_max_abs = max(self.range_max_abs, mx * 2.0 ** inf.act_shift)
        # every game that ran a round since the last clean poll is suspect: the ones in progress now + the finished ones not handed out yet
        self.clamp_window.on_event(e.status()[0][:, _abi.STC_GAMES_DONE])
        batch = dict(planes=e.features, split_features=(e.rows, e.N)) if e.features_split else {}  # (the re-calibration takes the stem's own layout)
        if inf.repair_range(ev, mx, slot=0, **batch):
            self.range_rescales += 1
        self._graph = None  # re-captured after any repair: never a replay across a change of InferenceNet.capture_state()
        self._announce_fallback()

    def harvest(self, with_moves=False):
        """Finished games as the reference actor emits them: [(game_seq: list[Transition], stats: dict)]
        (pipeline.py:283, :356-380).  pi_prob is float64 for Go and float32 for Gomoku like the reference.
        with_moves=True yields (game_seq, stats, moves): the game's move list as env.history holds it (flat actions, N*N = pass;
        a final resignation is not a history move, base.py:224-226) -- what to_sgf() needs (pipeline.py:276-281).
        Under a playout cap game_seq holds the full-search samples only; stats["game_length"] and the moves stay the whole game's and
        stats["num_full_samples"] (present only then) is len(game_seq)."""
        got = self.engine.harvest(with_moves=with_moves, with_class=self.playout_cap is not None)
        self._check_evaluator_range()
        states, pi, z, games = got[:4]
        full = got[-1].cpu().numpy() != 0 if self.playout_cap is not None else None
        extra = self.engine.last_extra
        if len(games) == 0:
            self.last_harvest_clamped = np.zeros(0, dtype=bool)
            return []
        states, pi, z = states.cpu().numpy(), pi.cpu().numpy(), z.cpu().numpy()
        moves = got[4].cpu().numpy() if with_moves else None
        out = []
        self.last_harvest_clamped = self.clamp_window.mask(games[:, _abi.GR_UID])
        for row, ex, clamped in zip(games, extra, self.last_harvest_clamped):
            s0, ln = int(row[_abi.GR_START]), int(row[_abi.GR_LENGTH])
            if clamped:
                # the game ran a round between a clamp event of the fp32-class evaluator and its repair: some of its searches may have
                # used a clamped activation where the reference's fp32 forward (pipeline.py:102-109) carries the value on
                self.clamped_games += 1
                if self.drop_clamped_games:
                    continue
            if int(ex[_abi.GX_STRADDLED]):
                # The game was in progress across a weight hot-swap -- impossible in the reference, whose actor only reloads between
                # games (pipeline.py:232-239).  It keeps the tag of the weights that STARTED it (pipeline.py:237 -> :271) and is
                # counted; drop_straddling_games=True discards it instead.
                self.straddled_games += 1
                if self.drop_straddling_games:
                    continue
            pis = pi[s0:s0 + ln].astype(np.float64) if self.game == "go" else pi[s0:s0 + ln]
            seq = [Transition(state=states[s0 + i].copy(), pi_prob=pis[i].copy(), value=float(z[s0 + i])) for i in range(ln)
                   if full is None or full[s0 + i]]
            # the threshold this very game was played with (pipeline.py:241-242, :379), exact double
            thr = float(np.array([ex[_abi.GX_THRESHOLD_LO], ex[_abi.GX_THRESHOLD_HI]], dtype=np.int32).view(np.float64)[0])
            stats = game_stats_from_row(row, self.game, self.komi, thr)
            stats["training_steps"] = int(row[_abi.GR_TRAINING_STEPS])  # weights in use when the game started (pipeline.py:237, :271, :492)
            if full is not None:
                stats["num_full_samples"] = len(seq)
            if clamped:
                stats["evaluator_clamped"] = True  # (only ever present on such a game: the reference's stats keys stay as they are)
            out.append((seq, stats, [int(m) for m in moves[s0:s0 + ln] if m >= 0]) if with_moves else (seq, stats))
        return out

    def game_sgf(self, stats, moves, date=""):
        """SGF text of a harvested game in the reference's format (go.py:202-210 / gomoku.py:149-157 through sgf_wrapper.make_sgf)."""
        from ..envs.base import PlayerMove
        from ..utils.sgf import make_sgf

        n = self.cfg.board_size
        hist = [PlayerMove("B" if i % 2 == 0 else "W", m) for i, m in enumerate(moves)]
        is_go = self.game == "go"
        return make_sgf(n, hist, stats["game_result"], ruleset="Chinese" if is_go else "", komi=self.komi if is_go else "", date=date)

    def counters(self, reset=False):
        return self.engine.counters(reset)


def load_checkpoint_state(path, allow_pickle=None):
    """Checkpoint dictionary of the learner (pipeline.py:597-606: 'network', 'training_steps', optimizer / scheduler state) from `path`.
    Loaded with weights_only=True: tensors, numbers, strings, containers -- no pickled code runs.  Only when the safe loader REJECTS the
    file's content (pickle.UnpicklingError: an object type outside its allow-list, e.g. a pickled scheduler object) and the caller opted
    in (allow_pickle=True, or the environment variable AZSP_ALLOW_PICKLE_CKPT=1) is the file re-read with the full unpickler, and that
    is logged.  I/O errors and corrupt files propagate; they are never retried with the unsafe loader."""
    import logging
    import os
    import pickle

    import collections

    try:  # MultiStepLR.state_dict() (training_go.py:273) holds its milestones as a collections.Counter: plain data, allow-listed
        with torch.serialization.safe_globals([collections.Counter, collections.OrderedDict]):
            return torch.load(path, map_location="cpu", weights_only=True)
    except pickle.UnpicklingError as e:
        if allow_pickle is None:
            allow_pickle = os.environ.get("AZSP_ALLOW_PICKLE_CKPT", "0") == "1"
        if not allow_pickle:
            raise
        logging.getLogger("alpha_zero_amd").warning("checkpoint %s needs the full unpickler (%s): loading with weights_only=False", path, e)
        return torch.load(path, map_location="cpu", weights_only=False)


def run_selfplay_actor_loop(seed, rank, network, device, data_queue, env, num_simulations, num_parallel, c_puct_base, c_puct_init,
                            warm_up_steps, check_resign_after_steps, disable_resign_ratio, save_sgf_dir=None, save_sgf_interval=0,
                            logs_dir=None, load_ckpt=None, log_level="INFO", var_ckpt=None, var_resign_threshold=None,
                            ckpt_event=None, stop_event=None, num_games=4096, net_dtype=torch.float32, harvest_every=64, binding=None,
                            playout_cap=None, leaf_symmetry=None, forced_playouts=None, gumbel=None, fpu_reduction=None):
    """Same role and argument list as the reference actor entry point (pipeline.py:166-189), extended by
    `num_games`: one call drives `num_games` games on `device` and puts (game_seq, stats) tuples on
    `data_queue` exactly as `num_games` reference actors would.  `net_dtype` defaults to the reference's evaluator precision (fp32,
    see SelfPlayActor).  `playout_cap`, `leaf_symmetry`, `forced_playouts`, `gumbel`, `fpu_reduction`: the opt-in search rules, SearchOptions.of; under a
    playout cap the queued game_seq hold the full-search samples only, and the queued pi rows are the rule's policy targets."""
    SearchOptions.of(leaf_symmetry, forced_playouts, gumbel=gumbel, playout_cap=playout_cap, num_simulations=num_simulations,
                     fpu_reduction=fpu_reduction)
    import os

    game = "go" if env.has_pass_move else "gomoku"
    training_steps = 0
    if load_ckpt is not None and os.path.exists(load_ckpt):  # pipeline.py:208-212
        st = load_checkpoint_state(load_ckpt)
        network.load_state_dict(st["network"])
        training_steps = st["training_steps"]
    thr = var_resign_threshold.value if (var_resign_threshold is not None and env.has_resign_move) else -1.0
    actor = SelfPlayActor(network, game=game, board_size=env.board_size, num_games=num_games, num_simulations=num_simulations,
                          num_parallel=num_parallel, c_puct_base=c_puct_base, c_puct_init=c_puct_init, warm_up_steps=warm_up_steps,
                          check_resign_after_steps=check_resign_after_steps, disable_resign_ratio=disable_resign_ratio,
                          resign_threshold=thr, komi=getattr(env, "komi", 7.5), num_to_win=getattr(env, "num_to_win", 5),
                          seed=seed, rank=rank, device=device, net_dtype=net_dtype, training_steps=training_steps, binding=binding,
                          num_stack=getattr(env, "num_stack", 8), playout_cap=playout_cap, leaf_symmetry=leaf_symmetry,
                          forced_playouts=forced_playouts, gumbel=gumbel, fpu_reduction=fpu_reduction)
    actor.drop_clamped_games = True  # the learner never sees a game that ran on a clamping evaluator (the reference's fp32 has no range)
    writer = None
    if logs_dir:  # per-actor statistics file with the reference's columns (pipeline.py:196, :268-271; logs/go/9x9/actor0.csv)
        from ..utils.csv_writer import CsvWriter
        from ..utils.sgf import get_time_stamp

        writer = CsvWriter(os.path.join(logs_dir, f"actor{rank}.csv"))
    last_ckpt, t_last, played_games = None, time.time(), 0
    while stop_event is None or not stop_event.is_set():
        if ckpt_event is not None and ckpt_event.is_set():  # the learner is writing a checkpoint (pipeline.py:228-230)
            time.sleep(0.001)
            continue
        if var_resign_threshold is not None and env.has_resign_move and var_resign_threshold.value != actor.resign_threshold:
            actor.set_resign_threshold(var_resign_threshold.value)  # pipeline.py:241-242: read before every game
        if var_ckpt is not None:
            new_ckpt = var_ckpt.value.decode("utf-8") if isinstance(var_ckpt.value, bytes) else str(var_ckpt.value)
            if new_ckpt != "" and new_ckpt != last_ckpt and os.path.exists(new_ckpt):  # pipeline.py:232-239
                st = load_checkpoint_state(new_ckpt)
                network.load_state_dict(st["network"])
                actor.set_network(network, st["training_steps"])
                last_ckpt = new_ckpt
        # Rounds in small chunks, polling the checkpoint event between them.  The reference actor queues every game that finished before
        # the event, drops the one game that ends while it is set (pipeline.py:264-267) and starts no new game until it clears
        # (pipeline.py:228-230).  Here: the moment the event is seen, whatever has finished so far is harvested and queued (those games
        # ended before it was noticed), then the engine pauses at the top of the loop -- no game ends during the event, none is dropped;
        # the games in progress resume under the new weights and are counted as straddling (SelfPlayActor.straddled_games).
        done_rounds, poll = 0, max(1, min(8, harvest_every))
        while done_rounds < harvest_every and not (ckpt_event is not None and ckpt_event.is_set()) and not (stop_event is not None and stop_event.is_set()):
            actor.run_rounds(min(poll, harvest_every - done_rounds))
            done_rounds += poll
            actor.poll_evaluator_range()  # two words: a clamp event is repaired within `poll` rounds, the games of the window are remembered
        want_sgf = bool(save_sgf_dir) and save_sgf_interval > 0 and os.path.isdir(save_sgf_dir)
        finished = actor.harvest(with_moves=want_sgf)
        now = time.time()
        if stop_event is not None and stop_event.is_set():
            break
        if want_sgf:  # every save_sgf_interval-th finished game is dumped like the reference does (pipeline.py:276-281)
            from ..utils.sgf import get_time_stamp as _ts

            for seq, stats, moves in finished:
                played_games += 1
                if played_games % save_sgf_interval == 0:
                    with open(os.path.join(save_sgf_dir, f"actor{rank}_{_ts(True)}_{played_games}.sgf"), "w") as f:
                        f.write(actor.game_sgf(stats, moves, date=_ts()))
            finished = [(seq, stats) for seq, stats, _ in finished]
        for seq, stats in finished:
            ts = stats.pop("training_steps")
            stats["time_per_game"] = round((now - t_last) * num_games / max(1, len(finished)), 4)
            stats["training_steps"] = ts  # key order of the reference's stats / CSV columns (pipeline.py:268-271)
            if writer is not None:
                writer.write({"datetime": get_time_stamp(), **stats})
            data_queue.put((seq, stats))
        if finished:
            t_last = now
    if writer is not None:
        writer.close()
