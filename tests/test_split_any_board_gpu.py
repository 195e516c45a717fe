"""The wave-per-tile stem of the fp32-class evaluator (k_stem_spg, csrc/az_stem_spg.h: azsp_stem_split / azsp_stem_split_exact on any
board) and the opt-in whole evaluator built on it (InferenceNet.use_split_any_board, SelfPlayActor(split_any_board=True)).

Checker = torch in fp64 on the CPU; the tailored stems for the bit-identity statements."""
import ctypes
import json
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from alpha_zero_amd.core.network import AlphaZeroNet, InferenceNet, split_weights_f16

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


def _stem_inputs(boards, n, C, seed, exact=False, cin=17):
    g = torch.Generator().manual_seed(seed)
    if exact:
        x = (torch.rand(boards, cin, n, n, generator=g) > 0.6).float()
    else:
        x = torch.randn(boards, cin, n, n, generator=g)
        x = torch.where(torch.rand(boards, cin, n, n, generator=g) < 0.5, torch.zeros(()), x.abs())  # half zeros
        x[:, :2] *= 37.0    # loud planes ...
        x[:, -2:] *= 3e-3   # ... and quiet ones
    w = torch.randn(C, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    b = torch.randn(C, generator=g) * 0.1
    return x, w, b


def _run_stem(dll, x, w, b, pad, exact=False, relu=1):
    """azsp_split_features -> azsp_stem_split (or _exact) with a private range record: (raw split-layout y as f16 words on the host, y as fp32
    [B,C,S,S], (events, max_abs) of the private record)."""
    B, cin, n, _ = x.shape
    C, S = w.shape[0], n + 2 * (pad - 1)
    feat = torch.zeros(dll.azsp_split_bytes(B, n, 32) // 2, dtype=torch.float16, device="cuda")
    ys = torch.zeros(dll.azsp_split_bytes(B, S, C) // 2, dtype=torch.float16, device="cuda")
    rec = torch.zeros(2, dtype=torch.int32, device="cuda")
    xd = x.cuda().contiguous()
    assert dll.azsp_split_features(xd.data_ptr(), feat.data_ptr(), B, n, cin, rec.data_ptr(), None) == 0
    w32 = torch.zeros(C, 32, 3, 3)
    w32[:, :cin] = w
    wsp, bb = split_weights_f16(w32).cuda(), b.float().cuda()
    stem = dll.azsp_stem_split_exact if exact else dll.azsp_stem_split
    assert stem(feat.data_ptr(), wsp.data_ptr(), bb.data_ptr(), ys.data_ptr(), B, n, C, pad, relu, rec.data_ptr(), None) == 0
    y = torch.empty(B, C, S, S, device="cuda").contiguous(memory_format=torch.channels_last)
    assert dll.azsp_split_layout(ys.data_ptr(), y.data_ptr(), B, S, C, 0, None, None) == 0
    torch.cuda.synchronize()
    r = rec.cpu()
    return ys.cpu(), y.cpu().contiguous(), (int(r[0]) & 0xFFFFFFFF, float(r[1:].view(torch.float32)[0]))


@pytest.mark.parametrize("n,pad,C", [(9, 1, 128), (9, 1, 64), (13, 3, 64)])
def test_gpu_wave_per_tile_stem_is_bit_identical_to_the_tailored_stems(n, pad, C):
    """k_stem_spg against the tailored stem of the same shape (k_conv3x3_sp<.., 4, NCG> with its corner phase, k_conv3x3_sp17<.., 4>):
    azsp_small_batch_waves(0) runs the tailored stem, a huge threshold the wave-per-tile one at any board count.  The raw hi / lo f16
    words are equal, on random fp32 planes (azsp_stem_split) and on 0 / 1 planes (azsp_stem_split_exact), and a private range record
    shows the same largest |v| (one channel's bias drives its outputs beyond f16's range in the second pass)."""
    from alpha_zero_amd import _lib

    dll = _lib.load().dll
    S = n + 2 * (pad - 1)
    old = dll.azsp_small_batch_waves(-1)
    try:
        for boards in (1, 2, 3, 5, 17):
            for exact in (False, True):
                for loud in (False, True):
                    x, w, b = _stem_inputs(boards, n, C, 700 + boards, exact)
                    if loud:
                        b[C - 3] = 3.0e5
                    dll.azsp_small_batch_waves(0)
                    ya, fa, ra = _run_stem(dll, x, w, b, pad, exact)
                    dll.azsp_small_batch_waves(HUGE)
                    yb, fb, rb = _run_stem(dll, x, w, b, pad, exact)
                    where = f"n={n} pad={pad} C={C} boards={boards} exact={exact} loud={loud}"
                    if not torch.equal(ya, yb):
                        d = (ya.view(boards, 2, C // 8, S * S, 8) != yb.view(boards, 2, C // 8, S * S, 8)).any(dim=4).any(dim=1).nonzero()
                        raise AssertionError(f"{where}: {len(d)} (board, chunk, position) cells differ; first {d[:12].tolist()}; "
                                             f"max |d| = {(fa - fb).abs().max().item():.3g}")
                    assert ra[1] == rb[1] and (ra[0] > 0) == (rb[0] > 0) == loud, (where, ra, rb)
                    assert (ra[1] > 65504.0) == loud, (where, ra)
    finally:
        dll.azsp_small_batch_waves(old)


@pytest.mark.parametrize("n,pad,C", [(19, 1, 64), (19, 1, 128), (19, 1, 256), (13, 1, 64), (15, 3, 64), (5, 1, 64), (7, 3, 64)])
def test_gpu_wave_per_tile_stem_on_boards_without_a_tailored_stem_vs_fp64(n, pad, C):
    """Shapes azsp_stem_split refused before, against relu(conv2d) in fp64: plane sizes 361, 169, 25 and 121 are no multiple of 16 (partial
    column tiles), pad 3 makes every position of the embedding margin an output.  Bound: the wave-per-tile convolution's own, 8e-7 of
    max |y| (the stem sums 9 x 17 products where the tower sums at least 9 x 64).  The exact entry on 0 / 1 planes gives the same bits
    as the general one, and (7, 3, 64) -- 9x9 planes, a tailored TOWER shape -- runs too."""
    from alpha_zero_amd import _lib

    dll = _lib.load().dll
    old = dll.azsp_small_batch_waves(-1)
    try:
        for boards in (1, 3):
            for thr in (old, HUGE):  # (no tailored stem for these shapes: the threshold must not matter)
                dll.azsp_small_batch_waves(thr)
                x, w, b = _stem_inputs(boards, n, C, 900 + boards)
                _, y, rec = _run_stem(dll, x, w, b, pad)
                ref = torch.relu(F.conv2d(x.double(), w.double(), b.double(), padding=pad))
                assert y.shape == ref.shape
                scale = ref.abs().max().item()
                err = (y.double() - ref).abs().max().item() / scale
                lib = torch.relu(F.conv2d(x.cuda(), w.cuda(), b.cuda(), padding=pad)).cpu()
                lib_err = (lib.double() - ref).abs().max().item() / scale
                _record("split_stem_generic_error.jsonl", dict(n=n, pad=pad, C=C, boards=boards, threshold=thr, err=err, library_fp32_err=lib_err))
                assert err <= 8e-7 and rec == (0, 0.0), (n, pad, C, boards, err, lib_err, rec)
            x, w, b = _stem_inputs(boards, n, C, 950 + boards, exact=True)
            y0, f0, _ = _run_stem(dll, x, w, b, pad)
            y1, f1, _ = _run_stem(dll, x, w, b, pad, exact=True)
            assert torch.equal(y0, y1), (n, pad, C, boards, (f0 - f1).abs().max().item())
            ref = torch.relu(F.conv2d(x.double(), w.double(), b.double(), padding=pad))
            assert (f1.double() - ref).abs().max().item() / ref.abs().max().item() <= 8e-7
    finally:
        dll.azsp_small_batch_waves(old)


def test_gpu_wave_per_tile_stem_range_record():
    """A stem bias of 3e5 on one channel at 19x19: every lane that holds that channel and at least one live position reports once into
    the CALLER'S record.  A wave is two column tiles (32 positions), a lane one position of each: 361 positions are 23 column tiles = 11
    full waves of 16 such lanes + a last wave with 9 live positions in its first tile and none in its second -- 185 events per board; the 7
    dead lanes of that wave, which the tower kernel would count (192), do not report.  The per-device default record stays empty.  The
    clamped outputs are 65504, the other channels untouched."""
    from alpha_zero_amd import _lib

    dll = _lib.load().dll
    old = dll.azsp_small_batch_waves(-1)
    ev, mx = ctypes.c_uint32(0), ctypes.c_float(0.0)
    try:
        assert dll.azsp_split_range_status(None, None, 1, None) == 0
        for boards in (1, 3):
            x, w, b = _stem_inputs(boards, 19, 64, 40 + boards)
            b[21] = 3.0e5
            _, y, rec = _run_stem(dll, x, w, b, 1)
            ref = F.conv2d(x.double(), w.double(), b.double(), padding=1)
            assert rec[0] == boards * (11 * 16 + 9) and rec[0] > 0 and abs(rec[1] - ref[:, 21].max().item()) <= 1.0, rec
            assert (y[:, 21] == 65504.0).all()
            others = [c for c in range(64) if c != 21]
            assert (y[:, others].double() - torch.relu(ref[:, others])).abs().max().item() <= 8e-7 * ref[:, others].abs().max().item()
            assert dll.azsp_split_range_status(ctypes.byref(ev), ctypes.byref(mx), 0, None) == 0
            assert (ev.value, mx.value) == (0, 0.0)
    finally:
        dll.azsp_small_batch_waves(old)


def _trained_like(net):
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):  # non-trivial running statistics, as after training
                m.running_mean.normal_(0, 0.2), m.running_var.uniform_(0.5, 1.5), m.weight.uniform_(0.7, 1.3), m.bias.normal_(0, 0.2)
    return net.eval()


@pytest.mark.parametrize("game,n,blocks", [("go", 19, 2), ("gomoku", 15, 1)])
def test_gpu_whole_evaluator_on_any_board_vs_fp64(game, n, blocks):
    """use_split_any_board on a 64-filter 19x19 Go net and a 15x15 Gomoku net (pad-3 stem, 19x19 planes): stem -> tower -> azsp_head_split,
    against the fp64 module next to the default path (split tower behind the library's stem and heads).  The project's rule for a
    hand-written fp32-class path (tests/test_split_tower.py, test_gpu_fp32_network_on_the_split_kernels): within 2e-4 of fp64 and at most
    4x + 2e-5 the default path's distance."""
    from alpha_zero_amd import _lib

    torch.manual_seed(3)
    A = n * n + (1 if game == "go" else 0)
    net = _trained_like(AlphaZeroNet((17, n, n), A, blocks, 64, 64, gomoku=game == "gomoku"))
    inf = InferenceNet(net, dtype=torch.float32, binding=_lib.load()).cuda()
    dll = inf.binding.dll
    old = dll.azsp_small_batch_waves(-1)
    out = []
    try:
        for boards in (1, 5):
            x = (torch.rand(boards, 17, n, n, generator=torch.Generator().manual_seed(boards)) > 0.6).float()
            with torch.no_grad():
                lg, v64 = net.double()(x.double())
            net.float()
            p64, v64 = torch.softmax(lg, -1), v64.squeeze(1)

            def dist(pv):
                return (pv[0].cpu().double() - p64).abs().max().item(), (pv[1].cpu().double() - v64).abs().max().item()

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
        dll.azsp_small_batch_waves(old)
        for d in out:
            _record("split_any_board_network_error.jsonl", d)


def test_gpu_any_board_exact_stem_on_engine_written_features_equals_the_general_stem():
    """At 19x19: the forward on an AZSP_FEAT_F16_SPLIT tensor as the engine writes it (azsp_stem_split_exact: hi plane only) gives bit for
    bit the outputs of the forward on the same planes as fp32 (azsp_split_features + azsp_stem_split) -- the 9x9 statement of
    test_gpu_stem_on_engine_written_features_equals_the_general_stem."""
    import engine_util as eu
    from alpha_zero_amd import _lib

    torch.manual_seed(3)
    net = _trained_like(AlphaZeroNet((17, 19, 19), 362, 2, 64, 64))
    inf = InferenceNet(net, dtype=torch.float32, binding=_lib.load()).cuda()
    inf.use_split_any_board = True
    old = inf.binding.dll.azsp_small_batch_waves(-1)
    try:
        for rows in (1, 5, 33):
            x = (torch.rand(rows, 17, 19, 19, generator=torch.Generator().manual_seed(rows)) > 0.6).float()
            p0, v0 = inf.forward_split(x.cuda().contiguous())
            p1, v1 = inf.forward_split(eu.split_features(x).cuda(), split_features=(rows, 19))
            p2, v2 = inf.forward_rows(eu.split_features(x).cuda(), "split", rows, 19)
            assert torch.equal(p0, p1) and torch.equal(v0, v1) and torch.equal(p0, p2) and torch.equal(v0, v2), (rows, float((p0 - p1).abs().max()))
    finally:
        inf.binding.dll.azsp_small_batch_waves(old)


def test_gpu_selfplay_actor_on_19x19_with_split_any_board():
    """SelfPlayActor(split_any_board=True) at 19x19: the engine writes AZSP_FEAT_F16_SPLIT, no fallback warning is raised, 40 captured
    rounds run without a range event, and the games they finish (10-move games) pass the game checks of engine_util."""
    import engine_util as eu
    from alpha_zero_amd import _abi, _lib
    from alpha_zero_amd.core.pipeline import SelfPlayActor

    torch.manual_seed(1)
    net = AlphaZeroNet((17, 19, 19), 362, 1, 64, 64)
    bnd = _lib.load()
    old = bnd.dll.azsp_small_batch_waves(-1)
    try:
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
    finally:
        bnd.dll.azsp_small_batch_waves(old)


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
    old = b.dll.azsp_small_batch_waves(-1)
    try:
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
    finally:
        b.dll.azsp_small_batch_waves(old)
