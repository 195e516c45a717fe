"""The wave-per-tile stem of the fp32-class evaluator (k_stem_spg, csrc/az_conv_spg.h: azsp_stem_split / azsp_stem_split_exact on any
board) and the opt-in whole evaluator built on it (InferenceNet.use_split_any_board, SelfPlayActor(split_any_board=True)).

Checker = torch in fp64 on the CPU; the tailored stems for the bit-identity statements.  Inputs, the stem driver and references are those of
tests/split_util.py."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

import split_util as su
from alpha_zero_amd.core.network import AlphaZeroNet, InferenceNet

pytestmark = pytest.mark.gpu
HUGE = 1 << 40


def _record(name, row):
    """Measured values: printed (pytest -s shows them), and appended as a JSON line to `name` in the directory AZSP_RESULTS_DIR names, if set."""
    print(json.dumps(row))
    out = os.environ.get("AZSP_RESULTS_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, name), "a") as f:
            f.write(json.dumps(row) + "\n")


@pytest.mark.parametrize("n,pad,C", [(9, 1, 128), (9, 1, 64), (13, 3, 64)])
def test_gpu_wave_per_tile_stem_is_bit_identical_to_the_tailored_stems(n, pad, C):
    """k_stem_spg against the tailored stem of the same shape (k_conv3x3_sp<.., 4, NCG> with its corner phase, k_conv3x3_sp17<.., 4>):
    azsp_small_batch_waves(0) runs the tailored stem, a huge threshold the wave-per-tile one at any board count.  The raw hi / lo f16
    words are equal, on random fp32 planes (azsp_stem_split) and on 0 / 1 planes (azsp_stem_split_exact), and a private range record
    shows the same largest |v| (one channel's bias drives its outputs beyond f16's range in the second pass)."""
    from alpha_zero_amd import _lib

    dll = _lib.load().dll
    S = n + 2 * (pad - 1)
    for boards in (1, 2, 3, 5, 17):
        for exact in (False, True):
            for loud in (False, True):
                x, w, b = su.stem_inputs(boards, n, C, 700 + boards, exact)
                if loud:
                    b[C - 3] = 3.0e5
                with su.small_batch_waves(dll, 0):
                    ya, fa, ra = su.split_stem(dll, x, w, b, pad, exact)
                with su.small_batch_waves(dll, HUGE):
                    yb, fb, rb = su.split_stem(dll, x, w, b, pad, exact)
                where = f"n={n} pad={pad} C={C} boards={boards} exact={exact} loud={loud}"
                su.assert_same_words(ya, yb, boards, C, S, where, fa, fb)
                assert ra[1] == rb[1] and (ra[0] > 0) == (rb[0] > 0) == loud, (where, ra, rb)
                assert (ra[1] > 65504.0) == loud, (where, ra)


@pytest.mark.parametrize("n,pad,C", [(19, 1, 64), (19, 1, 128), (19, 1, 256), (13, 1, 64), (15, 3, 64), (5, 1, 64), (7, 3, 64)])
def test_gpu_wave_per_tile_stem_on_boards_without_a_tailored_stem_vs_fp64(n, pad, C):
    """Shapes azsp_stem_split refused before, against relu(conv2d) in fp64: plane sizes 361, 169, 25 and 121 are no multiple of 16 (partial
    column tiles), pad 3 makes every position of the embedding margin an output.  Bound: the wave-per-tile convolution's own, 8e-7 of
    max |y| (the stem sums 9 x 17 products where the tower sums at least 9 x 64).  The exact entry on 0 / 1 planes gives the same bits
    as the general one, and (7, 3, 64) -- 9x9 planes, a tailored TOWER shape -- runs too."""
    from alpha_zero_amd import _lib

    dll = _lib.load().dll
    with su.small_batch_waves(dll) as old:
        for boards in (1, 3):
            for thr in (old, HUGE):  # (no tailored stem for these shapes: the threshold must not matter)
                dll.azsp_small_batch_waves(thr)
                x, w, b = su.stem_inputs(boards, n, C, 900 + boards)
                _, y, rec = su.split_stem(dll, x, w, b, pad)
                ref = su.ref64_conv(x, None, w, b, 1, padding=pad)
                assert y.shape == ref.shape
                err, lib_err = su.rel_err(y, ref), su.rel_err(su.library_conv(x, None, w, b, 1, padding=pad), ref)
                _record("split_stem_generic_error.jsonl", dict(n=n, pad=pad, C=C, boards=boards, threshold=thr, err=err, library_fp32_err=lib_err))
                assert err <= 8e-7 and rec == (0, 0.0), (n, pad, C, boards, err, lib_err, rec)
            x, w, b = su.stem_inputs(boards, n, C, 950 + boards, exact=True)
            y0, f0, _ = su.split_stem(dll, x, w, b, pad)
            y1, f1, _ = su.split_stem(dll, x, w, b, pad, exact=True)
            assert torch.equal(y0, y1), (n, pad, C, boards, (f0 - f1).abs().max().item())
            assert su.rel_err(f1, su.ref64_conv(x, None, w, b, 1, padding=pad)) <= 8e-7


def test_gpu_wave_per_tile_stem_range_record():
    """A stem bias of 3e5 on one channel at 19x19: every lane that holds that channel and at least one live position reports once into
    the CALLER'S record.  A wave is two column tiles (32 positions), a lane one position of each: 361 positions are 23 column tiles = 11
    full waves of 16 such lanes + a last wave with 9 live positions in its first tile and none in its second -- 185 events per board; the 7
    dead lanes of that wave, which the tower kernel would count (192), do not report.  The per-device default record stays empty.  The
    clamped outputs are 65504, the other channels untouched."""
    from alpha_zero_amd import _lib

    dll = _lib.load().dll
    with su.small_batch_waves(dll):
        su.default_record(dll, reset=1)
        for boards in (1, 3):
            x, w, b = su.stem_inputs(boards, 19, 64, 40 + boards)
            b[21] = 3.0e5
            _, y, rec = su.split_stem(dll, x, w, b, 1)
            ref = su.ref64_conv(x, None, w, b, 0)  # pre-activations
            assert rec[0] == boards * (11 * 16 + 9) and rec[0] > 0 and abs(rec[1] - ref[:, 21].max().item()) <= 1.0, rec
            assert (y[:, 21] == 65504.0).all()
            others = [c for c in range(64) if c != 21]
            assert (y[:, others].double() - torch.relu(ref[:, others])).abs().max().item() <= 8e-7 * ref[:, others].abs().max().item()
            assert su.default_record(dll) == (0, 0.0)


@pytest.mark.parametrize("game,n,blocks", [("go", 19, 2), ("gomoku", 15, 1)])
def test_gpu_whole_evaluator_on_any_board_vs_fp64(game, n, blocks):
    """use_split_any_board on a 64-filter 19x19 Go net and a 15x15 Gomoku net (pad-3 stem, 19x19 planes): stem -> tower -> azsp_head_split,
    against the fp64 module next to the default path (split tower behind the library's stem and heads).  The project's rule for a
    hand-written fp32-class path (tests/test_split_tower.py, test_gpu_fp32_network_on_the_split_kernels): within 2e-4 of fp64 and at most
    4x + 2e-5 the default path's distance."""
    from alpha_zero_amd import _lib

    torch.manual_seed(3)
    A = n * n + (1 if game == "go" else 0)
    net = su.trained_like(AlphaZeroNet((17, n, n), A, blocks, 64, 64, gomoku=game == "gomoku"))
    inf = InferenceNet(net, dtype=torch.float32, binding=_lib.load()).cuda()
    out = []
    try:
        with su.small_batch_waves(inf.binding.dll):
            for boards in (1, 5):
                x = (torch.rand(boards, 17, n, n, generator=torch.Generator().manual_seed(boards)) > 0.6).float()
                dist = su.dist_to_fp64(net, x)
                inf.use_split_any_board, inf._split = False, None
                assert not inf.supports_split_features(n, "cuda")
                d_off = dist(inf(x.cuda()))
                assert inf._split is not None
                inf.use_split_any_board, inf._split = True, None
                assert inf.supports_split_features(n, "cuda") and "hand-written" in inf.evaluator_path(n, "cuda")
                pv = inf(x.cuda())
                assert inf._split is not None, "the split kernels did not run"
                d_on = dist(pv)
                assert abs(pv[0].sum(1) - 1).max().item() <= 1e-5
                out.append(dict(game=game, n=n, boards=boards, opt_in_vs_fp64=d_on, default_vs_fp64=d_off))
                for k in (0, 1):
                    assert d_on[k] <= 2e-4 and d_on[k] <= 4 * d_off[k] + 2e-5, out[-1]
            assert inf.split_range_status(reset=True)[0] == 0
    finally:
        for d in out:
            _record("split_any_board_network_error.jsonl", d)


def test_gpu_any_board_exact_stem_on_engine_written_features_equals_the_general_stem():
    """At 19x19: the forward on an AZSP_FEAT_F16_SPLIT tensor as the engine writes it (azsp_stem_split_exact: hi plane only) gives bit for
    bit the outputs of the forward on the same planes as fp32 (azsp_split_features + azsp_stem_split) -- the 9x9 statement of
    test_gpu_stem_on_engine_written_features_equals_the_general_stem."""
    import engine_util as eu
    from alpha_zero_amd import _lib

    torch.manual_seed(3)
    net = su.trained_like(AlphaZeroNet((17, 19, 19), 362, 2, 64, 64))
    inf = InferenceNet(net, dtype=torch.float32, binding=_lib.load()).cuda()
    inf.use_split_any_board = True
    with su.small_batch_waves(inf.binding.dll):
        for rows in (1, 5, 33):
            x = (torch.rand(rows, 17, 19, 19, generator=torch.Generator().manual_seed(rows)) > 0.6).float()
            p0, v0 = inf.forward_split(x.cuda().contiguous())
            p1, v1 = inf.forward_split(eu.split_features(x).cuda(), split_features=(rows, 19))
            p2, v2 = inf.forward_rows(eu.split_features(x).cuda(), "split", rows, 19)
            assert torch.equal(p0, p1) and torch.equal(v0, v1) and torch.equal(p0, p2) and torch.equal(v0, v2), (rows, float((p0 - p1).abs().max()))


def test_gpu_selfplay_actor_on_19x19_with_split_any_board():
    """SelfPlayActor(split_any_board=True) at 19x19: the engine writes AZSP_FEAT_F16_SPLIT, no fallback warning is raised, 40 captured
    rounds run without a range event, and the games they finish (10-move games) pass the game checks of engine_util."""
    import engine_util as eu
    from alpha_zero_amd import _abi, _lib
    from alpha_zero_amd.core.pipeline import SelfPlayActor

    torch.manual_seed(1)
    net = AlphaZeroNet((17, 19, 19), 362, 1, 64, 64)
    bnd = _lib.load()
    with su.small_batch_waves(bnd.dll):
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            a = SelfPlayActor(net, game="go", board_size=19, num_games=8, num_simulations=8, num_parallel=4, split_any_board=True, use_graph=True,
                              binding=bnd, warm_up_steps=4, seed=3, engine_kw=dict(max_steps=10))
            assert a.cfg.feature_dtype == _abi.FEAT_F16_SPLIT and a.engine.features_split and a.split_features
            assert "hand-written" in a.evaluator_path and a.infer.use_split_any_board
            a.run_rounds(40)
            st, pi, z, rows = a.harvest_tensors()
        assert a.rounds == 40 and a.range_events == 0 and a.infer._split is not None
        assert len(rows) >= 1, "no game finished"
        stc, pic, zc = st.cpu().numpy(), pi.cpu().numpy(), z.cpu().numpy()
        assert stc.shape[1:] == (17, 19, 19) and np.allclose(pic.sum(axis=1), 1.0, atol=1e-4)
        occupied = (stc[:, 0] + stc[:, 1]).reshape(len(stc), 361) > 0
        assert not np.any((pic[:, :361] > 0) & occupied)  # no visit on an occupied point
        eu.assert_game_samples(rows, stc, zc, max_length=10)
        # a hot-swapped network gets the switch too
        a.set_network(AlphaZeroNet((17, 19, 19), 362, 1, 64, 64))
        assert a.infer.use_split_any_board and a.infer.supports_split_features(19, "cuda")


def test_gpu_parallel_uct_search_on_19x19_with_split_any_board():
    """parallel_uct_search (19x19, 32 simulations, P = 4) through a DeviceEvaluator on an opt-in InferenceNet: the device-resident loop
    (captured forward between the engine's tensors) and the host-callback loop give the same root child_N and move.  The search returns
    search_pi = child_N / sum(child_N) in float64, and both loops run the same 32 simulations, so bit-equal search_pi arrays are
    equal child_N (the drop-in search returns no raw counts)."""
    import engine_util as eu
    from alpha_zero_amd.core.evaluate import DeviceEvaluator
    from alpha_zero_amd.core.mcts_v2 import parallel_uct_search
    from alpha_zero_amd.envs.go import GoEnv

    torch.manual_seed(0)
    b = eu.gpu_binding()
    with su.small_batch_waves(b.dll):
        inf = InferenceNet(AlphaZeroNet((17, 19, 19), 362, 1, 64, 64).eval(), dtype=torch.float32, binding=b).cuda()
        inf.use_split_any_board = True
        ev = DeviceEvaluator(inf, use_graph=True)
        env = GoEnv(board_size=19)
        for mv in (72, 288, 60, 300):
            env.step(mv)
        inf._split = None
        r_dev = parallel_uct_search(env, ev, None, 19652.0, 1.25, 32, 4, deterministic=True)
        assert inf._split is not None and len(ev._graphs) >= 1
        r_cb = parallel_uct_search(env, lambda o, batched=False: ev(o, batched), None, 19652.0, 1.25, 32, 4, deterministic=True)
        assert r_dev[0] == r_cb[0] and np.array_equal(r_dev[1], r_cb[1]) and env.legal_actions[r_dev[0]] == 1
        assert inf.split_range_status(reset=True)[0] == 0
