"""Shared drivers for the tests of the fp32-class (split-precision) kernels: azsp_split_layout, azsp_split_features, azsp_conv3x3_split,
azsp_resblock_split, azsp_stem_split[_exact], azsp_split_range_* and azsp_small_batch_waves (include/azsp.h).  The same functions run
against the host twin (device "cpu") and libazsp.so on a MI355X (device "cuda").

Checker = torch in fp64 on the CPU, with the library's own fp32 convolution measured beside the kernel.  The error bounds of the tests
were measured on exactly the tensors the builders below return: generator, order of draws and scaling are part of their contract."""
import contextlib
import ctypes
from typing import NamedTuple

import torch
import torch.nn.functional as F

from alpha_zero_amd.core.network import AlphaZeroNet, split_weights_f16


# ---------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------
def _activations(g, boards, C, n, loud, scale=1.0):
    """Post-ReLU-like planes: half zeros, the first `loud` channels 37 x as large, the last `loud` 3e-3 x."""
    x = torch.randn(boards, C, n, n, generator=g) * scale
    x = torch.where(torch.rand(boards, C, n, n, generator=g) < 0.5, torch.zeros(()), x.abs())
    x[:, :loud] *= 37.0
    x[:, -loud:] *= 3e-3
    return x


def conv_inputs(boards, C, S, seed, scale=1.0):
    """x, r (residual), w, b of one convolution."""
    g = torch.Generator().manual_seed(seed)
    x = _activations(g, boards, C, S, C // 8, scale)
    r = torch.randn(boards, C, S, S, generator=g).abs() * scale
    w = torch.randn(C, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5
    b = torch.randn(C, generator=g) * 0.1
    return x, r, w, b


def resblock_inputs(boards, seed, S=17):
    """x, [w1, w2], [b1, b2] of one 64-filter ResNetBlock."""
    g = torch.Generator().manual_seed(seed)
    C = 64
    x = _activations(g, boards, C, S, C // 8)
    ws = [torch.randn(C, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5 for _ in range(2)]
    bs = [torch.randn(C, generator=g) * 0.1 for _ in range(2)]
    return x, ws, bs


def stem_inputs(boards, n, C, seed, exact=False, cin=17):
    """x (0 / 1 planes if exact, else activations), w, b of a stem with `cin` input planes on an n x n board."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(boards, cin, n, n, generator=g) > 0.6).float() if exact else _activations(g, boards, cin, n, 2)
    w = torch.randn(C, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    b = torch.randn(C, generator=g) * 0.1
    return x, w, b


# ---------------------------------------------------------------------------------------------------
# layout
# ---------------------------------------------------------------------------------------------------
def _ptr(t):
    return None if t is None else t.data_ptr()


def _split_zeros(dll, B, S, C, device):
    n = dll.azsp_split_bytes(B, S, C) // 2
    assert n == B * 2 * S * S * C
    return torch.zeros(n, dtype=torch.float16, device=device)


def to_split(dll, t, device, rec=None):
    """fp32 [B,C,S,S] -> the flat f16 split tensor on `device`; out-of-range values go to the record `rec` (None = the default record)."""
    B, C, S, _ = t.shape
    tc = t.to(device).contiguous(memory_format=torch.channels_last)
    ts = _split_zeros(dll, B, S, C, device)
    assert dll.azsp_split_layout(tc.data_ptr(), ts.data_ptr(), B, S, C, 1, _ptr(rec), None) == 0
    return ts


def from_split(dll, ys, B, S, C):
    """The flat f16 split tensor -> fp32 [B,C,S,S] on the host."""
    y = torch.empty(B, C, S, S, device=ys.device, memory_format=torch.channels_last)
    assert dll.azsp_split_layout(ys.data_ptr(), y.data_ptr(), B, S, C, 0, None, None) == 0
    if ys.is_cuda:
        torch.cuda.synchronize()
    return y.cpu().contiguous()


def to_split_features(dll, x, device, rec=None):
    """fp32 observation planes [B,cin,n,n] (cin <= 32) -> the split tensor padded to 32 channels that the stem kernels read."""
    B, cin, n, _ = x.shape
    xd = x.to(device).contiguous()
    feat = _split_zeros(dll, B, n, 32, device)
    assert dll.azsp_split_features(xd.data_ptr(), feat.data_ptr(), B, n, cin, _ptr(rec), None) == 0
    return feat


def split_params(w, b, device):
    """Folded fp32 weights and bias of one convolution as the kernels take them: (hi / lo f16 weights, fp32 bias)."""
    return split_weights_f16(w).to(device), b.float().to(device)


# ---------------------------------------------------------------------------------------------------
# launch drivers: one per entry point
# ---------------------------------------------------------------------------------------------------
class SplitConv(NamedTuple):
    raw: torch.Tensor   # the output in the split layout: f16 words on the host
    y: torch.Tensor     # the same joined to fp32 [B,C,S,S]
    roundtrip: float    # layout round-trip error of the input x, relative


def split_conv(bnd, x, r, w, b, relu, device):
    """x, r (or None): fp32 [B,C,S,S] -> azsp_split_layout -> azsp_conv3x3_split -> azsp_split_layout."""
    B, C, S, _ = x.shape
    dll = bnd.dll
    xs, ys = to_split(dll, x, device), _split_zeros(dll, B, S, C, device)
    rs = to_split(dll, r, device) if r is not None else None
    wsp, bb = split_params(w, b, device)
    assert dll.azsp_conv3x3_split(xs.data_ptr(), wsp.data_ptr(), bb.data_ptr(), _ptr(rs), ys.data_ptr(), B, S, C, relu, None, None) == 0
    y = from_split(dll, ys, B, S, C)
    # the layout round trip of the input itself: 22-bit significands.  |v - hi - lo / 2048| <= 2^-22 |v| (+ the fp32 rounding of the
    # join); below f16's normal range the lo half is a multiple of 2^-24 / 2048 = 2^-35: the excess over that absolute floor, relative to |v|
    back = from_split(dll, xs, B, S, C)
    rt = (((back - x).abs() - 2.0 ** -35).clamp_min(0) / x.abs().clamp_min(1e-30)).max().item()
    return SplitConv(ys.cpu(), y, rt)


def split_resblock(bnd, x, ws, bs, device):
    """One ResNetBlock both ways: (fused y, two-launch y) in the split layout, as raw f16 tensors, + the fused result as fp32 [B,C,S,S]."""
    B, C, S, _ = x.shape
    dll = bnd.dll
    xs = to_split(dll, x, device)
    ms, y2, yf = (_split_zeros(dll, B, S, C, device) for _ in range(3))
    (w1, b1), (w2, b2) = (split_params(w, b, device) for w, b in zip(ws, bs))
    assert dll.azsp_conv3x3_split(xs.data_ptr(), w1.data_ptr(), b1.data_ptr(), None, ms.data_ptr(), B, S, C, 1, None, None) == 0
    assert dll.azsp_conv3x3_split(ms.data_ptr(), w2.data_ptr(), b2.data_ptr(), xs.data_ptr(), y2.data_ptr(), B, S, C, 1, None, None) == 0
    assert dll.azsp_resblock_split(xs.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), yf.data_ptr(), B, S, C, None, None) == 0
    return yf, y2, from_split(dll, yf, B, S, C)


def split_stem(dll, x, w, b, pad, exact=False, relu=1, device="cuda"):
    """azsp_split_features -> azsp_stem_split (or _exact) on `device` with a private range record: (raw split-layout y as f16 words on the
    host, y as fp32 [B,C,S,S], (events, max_abs) of the private record)."""
    B, cin, n, _ = x.shape
    C, S = w.shape[0], n + 2 * (pad - 1)
    rec = new_record(device)
    feat, ys = to_split_features(dll, x, device, rec), _split_zeros(dll, B, S, C, device)
    w32 = torch.zeros(C, 32, 3, 3)
    w32[:, :cin] = w
    wsp, bb = split_params(w32, b, device)
    stem = dll.azsp_stem_split_exact if exact else dll.azsp_stem_split
    assert stem(feat.data_ptr(), wsp.data_ptr(), bb.data_ptr(), ys.data_ptr(), B, n, C, pad, relu, rec.data_ptr(), None) == 0
    y = from_split(dll, ys, B, S, C)
    return ys.cpu(), y, read_record(rec)


# ---------------------------------------------------------------------------------------------------
# references and comparisons
# ---------------------------------------------------------------------------------------------------
def ref64_conv(x, r, w, b, relu, padding=1):
    y = F.conv2d(x.double(), w.double(), b.double(), padding=padding)
    if r is not None:
        y = y + r.double()
    return torch.relu(y) if relu else y


def ref64_resblock(x, ws, bs):
    return ref64_conv(ref64_conv(x, None, ws[0], bs[0], 1), x, ws[1], bs[1], 1)


def library_conv(x, r, w, b, relu, padding=1):
    """The library's fp32 convolution on the GPU: its error is recorded beside the kernel's."""
    y = F.conv2d(x.cuda(), w.cuda(), b.cuda(), padding=padding)
    if r is not None:
        y = y + r.cuda()
    return (torch.relu(y) if relu else y).cpu()


def rel_err(y, ref):
    """max |y - ref| relative to max |ref|."""
    return (y.double() - ref).abs().max().item() / ref.abs().max().item()


def assert_same_words(ya, yb, boards, C, S, where, fa=None, fb=None):
    """Two outputs in the split layout are equal word for word; if not: which (board, chunk of 8 channels, position) cells differ."""
    if torch.equal(ya, yb):
        return
    bad = (ya.view(boards, 2, C // 8, S * S, 8) != yb.view(boards, 2, C // 8, S * S, 8)).any(dim=4).any(dim=1).nonzero()  # [board, chunk, position]
    msg = (f"{where}: {len(bad)} (board, chunk, position) cells differ; first {bad[:12].tolist()}; boards {sorted(set(bad[:, 0].tolist()))[:20]}; "
           f"rows {sorted(set((bad[:, 2] // S).tolist()))[:20]}")
    if fa is not None and fb is not None:  # the joined fp32 views of ya and yb
        msg += f"; max |d| = {(fa - fb).abs().max().item():.3g}"
    raise AssertionError(msg)


# ---------------------------------------------------------------------------------------------------
# range record
# ---------------------------------------------------------------------------------------------------
def new_record(device):
    """A caller-owned range record (`range_rec_dev` of the azsp_*_split entries): uint32 events, fp32 largest |v|."""
    return torch.zeros(2, dtype=torch.int32, device=device)


def read_record(rec):
    """(events, max_abs) of a caller-owned record."""
    if rec.is_cuda:
        torch.cuda.synchronize()
    r = rec.cpu()
    return int(r[0]) & 0xFFFFFFFF, float(r[1:].view(torch.float32)[0])


def default_record(dll, reset=0):
    """(events, max_abs) of the library's per-device default record (azsp_split_range_status)."""
    ev, mx = ctypes.c_uint32(0), ctypes.c_float(0.0)
    assert dll.azsp_split_range_status(ctypes.byref(ev), ctypes.byref(mx), reset, None) == 0
    return ev.value, mx.value


# ---------------------------------------------------------------------------------------------------
# the small-batch switch
# ---------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def small_batch_waves(dll, n=-1):
    """azsp_small_batch_waves(n) for the duration of the block (a negative n changes nothing), the previous value back on the way out;
    yields that previous value.  0 runs the tailored kernels at every board count, a huge value the wave-per-tile ones."""
    old = dll.azsp_small_batch_waves(n)
    try:
        yield old
    finally:
        dll.azsp_small_batch_waves(old)


# ---------------------------------------------------------------------------------------------------
# networks
# ---------------------------------------------------------------------------------------------------
def trained_like(net):
    """Non-trivial BatchNorm running statistics, as after training; returns net.eval()."""
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.2), m.running_var.uniform_(0.5, 1.5), m.weight.uniform_(0.7, 1.3), m.bias.normal_(0, 0.2)
    return net.eval()


def go9_net(filters, blocks, seed=3):
    torch.manual_seed(seed)
    return trained_like(AlphaZeroNet((17, 9, 9), 82, blocks, filters, 128))


def gomoku13_net(filters, blocks, seed=3, fc=64):
    torch.manual_seed(seed)
    return trained_like(AlphaZeroNet((17, 13, 13), 169, blocks, filters, fc, gomoku=True))


def dist_to_fp64(net, x):
    """The module evaluated in fp64 on x; returns dist((priors, values)) -> (max |dp|, max |dv|) against its softmax priors and values."""
    with torch.no_grad():
        lg, v64 = net.double()(x.double())
    net.float()  # (exact: the parameters were fp32)
    p64, v64 = torch.softmax(lg, -1), v64.squeeze(1)

    def dist(pv):
        return (pv[0].cpu().double() - p64).abs().max().item(), (pv[1].cpu().double() - v64).abs().max().item()

    return dist
