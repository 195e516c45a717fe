"""Exact-operand tier of the evaluator kernels (include/azsp.h): operands are chosen so that every product and every partial sum of a
kernel is exactly representable, whatever the summation order, MFMA shape, tile or workgroup.  The kernel must then return the correctly
rounded exact value BIT FOR BIT: the comparisons below are torch.equal, no tolerance.  A dropped term, a swapped tap, a bled padding cell,
a wrong rounding mode or a stale bias changes at least one bit.

Rule of the tier: operands exact, comparison bitwise, preconditions asserted.  Every driver asserts its precondition on the very tensors
it launches with (worst-case sum, integer hi planes, non-zero lo planes, rounded / tie shares, logit spread), so that a failed equality is
the kernel's fault and never the generator's.  The same drivers run against the host twin (device "cpu") and libazsp.so (device "cuda"),
in the way split_util.py's do.

A batch is built from at most PATTERNS distinct boards, board i = pattern (7 i) % PATTERNS: the fp64 reference is computed on the
patterns and indexed, which also re-checks that a board's result does not depend on the batch around it."""
import ctypes
import functools
from typing import NamedTuple

import torch
import torch.nn.functional as F

import engine_util as eu
import split_util as su

PATTERNS = 24
BITS_INT = 20           # integer operands: worst-case sum < 2^20, four bits under fp32's 24
CAP_CARRY = 2.0 ** 22   # operands with lo halves: 2048 * worst-case sum (the fp32 partial sums and the 22-bit output format)


class Fmt(NamedTuple):
    name: str
    dtype: torch.dtype
    bits: int   # significand bits, the hidden one included
    rmax: int   # |bias|, |residual| <= rmax are integers exactly representable; outputs from rmax up are rounded
    f16: int


BF16 = Fmt("bf16", torch.bfloat16, 8, 256, 0)
F16 = Fmt("f16", torch.float16, 11, 2048, 1)


def pattern_index(boards):
    return (7 * torch.arange(boards)) % PATTERNS


def _sync(device):
    if device != "cpu":
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------
# what "exact" means: quanta, worst cases, rounding shares
# ---------------------------------------------------------------------------------------------------
def quantum(t):
    """The largest power of two that divides every entry of the (dyadic, fp64) tensor t; inf for an all-zero tensor."""
    v = t.double().flatten()
    v = v[v != 0]
    if v.numel() == 0:
        return float("inf")
    m, e = torch.frexp(v)
    k = (m.abs() * 2.0 ** 53).to(torch.int64)   # 53-bit significand as an integer
    low = (k & -k).double()                       # its lowest set bit
    return float((low * torch.exp2((e - 53).double())).min())


def assert_sums_exact(worst, q, bits, what):
    """Every partial sum of terms that are multiples of q and whose absolute values add up to at most `worst` is a multiple of q below
    worst: exactly representable with `bits` significand bits when worst / q < 2^bits."""
    w = float(worst.max()) if torch.is_tensor(worst) else float(worst)
    assert w / q < 2.0 ** bits, f"{what}: worst-case sum {w:.6g} at quantum {q:.3g} needs {w / q:.4g} >= 2^{bits} steps: the generator is wrong, not the kernel"


def rounding_shares(ref, fmt):
    """(share of the entries of ref that are not representable in fmt, share that lie exactly half way between two neighbours)."""
    err = (ref - ref.float().to(fmt.dtype).double()).abs()
    _, e = torch.frexp(ref.abs())
    half = torch.exp2((e - fmt.bits - 1).double())  # |v| in [2^(e-1), 2^e): neighbours are 2^(e-bits) apart
    return float((err > 0).double().mean()), float(((err == half) & (err > 0)).double().mean())


def assert_rounding_is_tested(ref, fmt, what, rounded=0.25, ties=0.01):
    nr, nt = rounding_shares(ref, fmt)
    assert nr >= rounded and nt >= ties, f"{what}: {nr:.3%} of the outputs round and {nt:.3%} are ties in {fmt.name}: the rounding mode is not tested"
    assert float(ref.abs().max()) >= fmt.rmax and float(ref.abs().max()) < 65504.0


def assert_same_cells(got, want, where):
    """got == want element for element ([boards, C, S, S], same dtype); if not: the first differing (board, channel, row, column) cells,
    how many differ per row and per column, and got versus wanted."""
    assert got.shape == want.shape and got.dtype == want.dtype, (where, got.shape, want.shape, got.dtype, want.dtype)
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero()
    S = got.shape[2]
    first = [(tuple(c.tolist()), float(got[tuple(c)]), float(want[tuple(c)])) for c in bad[:8]]
    rows, cols = torch.bincount(bad[:, 2], minlength=S).tolist(), torch.bincount(bad[:, 3], minlength=got.shape[3]).tolist()
    raise AssertionError(f"{where}: {len(bad)} of {got.numel()} cells differ; first (board, channel, row, column), got, wanted: {first}; per row {rows}; "
                         f"per column {cols}; boards {sorted(set(bad[:, 0].tolist()))[:16]}; channels {sorted(set(bad[:, 1].tolist()))[:16]}; "
                         f"max |d| = {(got.double() - want.double()).abs().max().item():.6g}")


def assert_same_rows(got, want, where):
    """The same for [boards, n] outputs (head planes, bias_act rows)."""
    assert_same_cells(got.reshape(got.shape[0], 1, 1, -1), want.reshape(want.shape[0], 1, 1, -1), where)


def _conv64(x, w, pad=1):
    return F.conv2d(x.double(), w.double(), None, padding=pad)


_refs = {}


def _per_pattern(fn, idx, key):
    """fn(pattern indices) -> reference rows, computed on the distinct patterns of idx only -- once per `key` and set of patterns, shared by
    the cases that need it and never written to -- and indexed back to the batch."""
    uniq, inv = torch.unique(idx, return_inverse=True)
    key = (key, tuple(uniq.tolist()))
    if key not in _refs:
        _refs[key] = fn(uniq)
    return _refs[key][inv]


# ---------------------------------------------------------------------------------------------------
# generators: integer operands (lower-precision kernels and the fp32-class ones)
# ---------------------------------------------------------------------------------------------------
def _int_weights(g, shape, k, skew=0.15):
    """k * {-2..2}, a share `skew` of the negative ones turned positive: the outputs lean to the positive side, so that the ReLU leaves
    enough of them in the rounding range."""
    u = torch.randint(-2, 3, shape, generator=g).double()
    return k * torch.where((u < 0) & (torch.rand(shape, generator=g) < skew), -u, u)


def _int_acts(g, shape, top=3):
    x = torch.randint(1, top + 1, shape, generator=g).double()
    return torch.where(torch.rand(shape, generator=g) < 0.5, torch.zeros((), dtype=torch.float64), x)


def int_scale(C, thr):
    """The weight scale at which the convolution's standard deviation is about 2.5 thr: sigma = k sqrt(9 C / 2 * E[x^2 | x > 0] E[u^2])
    with E[x^2 | x > 0] = 14 / 3 for x in 1..3 and E[u^2] = 2 for u in -2..2."""
    return max(1, round(2.5 * thr / (9 * C / 2 * 14 / 3 * 2) ** 0.5))


@functools.lru_cache(maxsize=None)
def int_conv_operands(S, C, fmt_name, seed):
    """x [PATTERNS,C,S,S] in 0..3 (half zero), r integers in -rmax..rmax, w [C,C,3,3] = k {-2..2}, b integers in -rmax..rmax: fp64."""
    fmt = BF16 if fmt_name == "bf16" else F16
    g = torch.Generator().manual_seed(seed)
    x = _int_acts(g, (PATTERNS, C, S, S))
    r = torch.randint(-fmt.rmax, fmt.rmax + 1, (PATTERNS, C, S, S), generator=g).double()
    w = _int_weights(g, (C, C, 3, 3), int_scale(C, fmt.rmax))
    b = torch.randint(-fmt.rmax, fmt.rmax + 1, (C,), generator=g).double()
    return x, r, w, b


def int_conv_reference(x, r, w, b, relu, key=None):
    """(fp64 result, worst-case sum) of one convolution on integer operands; the two convolutions are kept under `key`."""
    if key is None or key not in _refs:
        base = _conv64(x, w), _conv64(x.abs(), w.abs())
        if key is not None:
            _refs[key] = base
    else:
        base = _refs[key]
    y, worst = base[0] + b.view(1, -1, 1, 1), base[1] + b.abs().view(1, -1, 1, 1)
    if r is not None:
        y, worst = y + r, worst + r.abs()
    return (torch.relu(y) if relu else y), worst


def assert_integers(what, *ts):
    for t in ts:
        if t is not None:
            assert torch.equal(t, t.round()), f"{what}: operands must be integers"


# ---------------------------------------------------------------------------------------------------
# tiled layout (bf16 / f16 evaluator)
# ---------------------------------------------------------------------------------------------------
def to_tiled(dll, t, fmt, device):
    """[B,C,S,S] exact values -> the flat tiled tensor of fmt on `device` (the conversion must be lossless)."""
    B, C, S, _ = t.shape
    tc = t.to(fmt.dtype)
    assert torch.equal(tc.double(), t.double()), "operand not representable in " + fmt.name
    tc = tc.to(device).contiguous(memory_format=torch.channels_last)
    out = torch.zeros(dll.azsp_tiled_bytes(B, S, C) // 2, dtype=fmt.dtype, device=device)
    assert dll.azsp_tile_layout(tc.data_ptr(), out.data_ptr(), B, S, C, 1, None) == 0
    return out


def from_tiled(dll, yt, B, S, C):
    """The flat tiled tensor -> [B,C,S,S] of its dtype on the host: every valid row, nothing masked."""
    y = torch.empty(B, C, S, S, dtype=yt.dtype, device=yt.device).contiguous(memory_format=torch.channels_last)
    assert dll.azsp_tile_layout(yt.data_ptr(), y.data_ptr(), B, S, C, 0, None) == 0
    _sync(yt.device.type)
    return y.cpu().contiguous()


def pack_taps(w, fmt, device, cin_pad=None):
    """[Cout,Cin,3,3] -> [9 taps][Cout][Cin (zero padded to cin_pad)] of fmt."""
    Co, Ci = w.shape[:2]
    wp = torch.zeros(9, Co, cin_pad or Ci, dtype=torch.float64)
    wp[:, :, :Ci] = w.permute(2, 3, 0, 1).reshape(9, Co, Ci)
    out = wp.to(fmt.dtype)
    assert torch.equal(out.double(), wp), "weight not representable in " + fmt.name
    return out.contiguous().to(device)


def tiled_conv_exact(bnd, device, S, C, boards, fmt, res, relu, seed=11):
    """azsp_conv3x3_tiled[_f16] on integer operands == RNE(fp64 convolution), bit for bit over every valid row."""
    dll = bnd.dll
    x, r, w, b = int_conv_operands(S, C, fmt.name, seed)
    idx = pattern_index(boards)
    where = f"conv3x3_tiled {fmt.name} S={S} C={C} boards={boards} res={res} relu={relu}"
    assert_integers(where, x, r, w, b)
    ref, worst = int_conv_reference(x, r if res else None, w, b, relu, key=("tiled_conv", S, C, fmt.name, seed))
    assert_sums_exact(worst, 1.0, BITS_INT, where)
    assert_rounding_is_tested(ref, fmt, where)
    xt, yt = to_tiled(dll, x[idx], fmt, device), torch.zeros(dll.azsp_tiled_bytes(boards, S, C) // 2, dtype=fmt.dtype, device=device)
    rt = to_tiled(dll, r[idx], fmt, device) if res else None
    wp, bb = pack_taps(w, fmt, device), b.float().to(device)
    conv = dll.azsp_conv3x3_tiled_f16 if fmt.f16 else dll.azsp_conv3x3_tiled
    assert conv(xt.data_ptr(), wp.data_ptr(), bb.data_ptr(), rt.data_ptr() if res else None, yt.data_ptr(), boards, S, C, relu, None) == 0
    assert_same_cells(from_tiled(dll, yt, boards, S, C), ref.float().to(fmt.dtype)[idx], where)


@functools.lru_cache(maxsize=None)
def int_block_operands(S, C, seed):
    """x, [w1, w2], [b1, b2] of a bf16 ResNetBlock: conv1 at the scale that puts the intermediate into bf16's rounding range, conv2 with
    weights in -2..2 so that conv(|mid|, |w2|) stays below 2^20."""
    g = torch.Generator().manual_seed(seed)
    x = _int_acts(g, (PATTERNS, C, S, S))
    ws = [_int_weights(g, (C, C, 3, 3), max(1, int_scale(C, BF16.rmax) // 6), skew=0.05), _int_weights(g, (C, C, 3, 3), 1, skew=0.02)]
    bs = [torch.randint(-256, 257, (C,), generator=g).double() for _ in range(2)]
    return x, ws, bs


def tiled_resblock_exact(bnd, device, S, C, boards, seed=12):
    """azsp_resblock_tiled, out of place and in place, == RNE(conv2(RNE(relu(conv1 x + b1))) + b2 + x), the intermediate rounded to bf16
    by the same round-to-nearest-even; precondition on conv(|mid|, |w2|) as well."""
    dll, fmt = bnd.dll, BF16
    x, ws, bs = int_block_operands(S, C, seed)
    idx = pattern_index(boards)
    where = f"resblock_tiled S={S} C={C} boards={boards}"
    assert_integers(where, x, *ws, *bs)
    mid64, worst1 = int_conv_reference(x, None, ws[0], bs[0], 1, key=("tiled_block1", S, C, seed))
    assert_sums_exact(worst1, 1.0, BITS_INT, where + " conv1")
    assert_rounding_is_tested(mid64, fmt, where + " intermediate", rounded=0.02, ties=0.005)  # (chosen: conv2's 2^20 cap keeps the intermediate small)
    mid = mid64.float().to(fmt.dtype).double()
    ref, worst2 = int_conv_reference(mid, x, ws[1], bs[1], 1, key=("tiled_block2", S, C, seed))
    assert_integers(where, mid)
    assert_sums_exact(worst2, 1.0, BITS_INT, where + " conv2")
    assert_rounding_is_tested(ref, fmt, where)
    want = ref.float().to(fmt.dtype)[idx]
    xt, yt = to_tiled(dll, x[idx], fmt, device), torch.zeros(dll.azsp_tiled_bytes(boards, S, C) // 2, dtype=fmt.dtype, device=device)
    wps, bbs = [pack_taps(w, fmt, device) for w in ws], [b.float().to(device) for b in bs]
    args = (wps[0].data_ptr(), bbs[0].data_ptr(), wps[1].data_ptr(), bbs[1].data_ptr())
    assert dll.azsp_resblock_tiled(xt.data_ptr(), *args, yt.data_ptr(), boards, S, C, None) == 0
    assert_same_cells(from_tiled(dll, yt, boards, S, C), want, where + " out of place")
    assert_same_cells(from_tiled(dll, xt, boards, S, C), x[idx].to(fmt.dtype), where + " input left alone")
    assert dll.azsp_resblock_tiled(xt.data_ptr(), *args, xt.data_ptr(), boards, S, C, None) == 0
    assert_same_cells(from_tiled(dll, xt, boards, S, C), want, where + " in place")


@functools.lru_cache(maxsize=None)
def int_stem_operands(n, C, fmt_name, seed, cin=17):
    """0 / 1 planes [PATTERNS,cin,n,n], integer weights [C,cin,3,3] = k {-2..2} and an integer bias."""
    fmt = BF16 if fmt_name == "bf16" else F16
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(PATTERNS, cin, n, n, generator=g) > 0.6).double()
    # int_scale's rule with 0.4 * 9 cin active terms of x^2 = 1
    k = max(1, round(2.5 * fmt.rmax / (0.4 * 9 * cin * 2) ** 0.5))
    w = _int_weights(g, (C, cin, 3, 3), k)
    b = torch.randint(-fmt.rmax, fmt.rmax + 1, (C,), generator=g).double()
    return x, w, b


def tiled_stem_exact(bnd, device, n, C, pad, boards, fmt, relu=1, seed=13):
    """azsp_stem_tiled[_f16]: 0 / 1 planes in the engine's tiled feature encoding, integer weights and bias."""
    dll = bnd.dll
    x, w, b = int_stem_operands(n, C, fmt.name, seed)
    idx = pattern_index(boards)
    So = n + 2 * (pad - 1)
    where = f"stem_tiled {fmt.name} board={n} C={C} pad={pad} boards={boards} relu={relu}"
    assert_integers(where, w, b)
    assert bool(((x == 0) | (x == 1)).all())
    ref = _conv64(x, w, pad) + b.view(1, -1, 1, 1)
    ref = torch.relu(ref) if relu else ref
    assert_sums_exact(_conv64(x, w.abs(), pad) + b.abs().view(1, -1, 1, 1), 1.0, BITS_INT, where)
    assert_rounding_is_tested(ref, fmt, where, rounded=0.1)  # (chosen: the margin of a pad-3 plane holds little more than the bias)
    feat = eu.tile_features(x[idx].float(), fmt.dtype).to(device)
    yt = torch.zeros(dll.azsp_tiled_bytes(boards, So, C) // 2, dtype=fmt.dtype, device=device)
    wp, bb = pack_taps(w, fmt, device, cin_pad=32), b.float().to(device)
    stem = dll.azsp_stem_tiled_f16 if fmt.f16 else dll.azsp_stem_tiled
    assert stem(feat.data_ptr(), wp.data_ptr(), bb.data_ptr(), yt.data_ptr(), boards, n, C, pad, relu, None) == 0
    assert_same_cells(from_tiled(dll, yt, boards, So, C), ref.float().to(fmt.dtype)[idx], where)


@functools.lru_cache(maxsize=None)
def head_tiled_operands(S, C, seed):
    """Tower output in 0..4 (half zero), 1x1 weights [3,C] and biases that are multiples of 1/8."""
    g = torch.Generator().manual_seed(seed)
    x = _int_acts(g, (PATTERNS, C, S, S), top=4)
    hw = torch.randint(-16, 17, (3, C), generator=g).double() / 8
    hb = torch.randint(-64, 65, (3,), generator=g).double() / 8
    return x, hw, hb


def tiled_head_exact(bnd, device, S, C, boards, fmt, strided, seed=14):
    """azsp_head_tiled[_f16], npol 2 + nval 1: out == RNE(relu(sum_c w x + bias)); rows dense (strided = False) or a multiple of 16
    elements apart, in which case the padding columns must come back untouched (the header leaves zeroing them to the caller)."""
    dll = bnd.dll
    x, hw, hb = head_tiled_operands(S, C, seed)
    idx = pattern_index(boards)
    P2 = S * S
    where = f"head_tiled {fmt.name} S={S} C={C} boards={boards} strided={strided}"
    assert_integers(where, x, hw * 8, hb * 8)
    ref = torch.relu(torch.einsum("bcp,lc->blp", x.reshape(PATTERNS, C, P2), hw) + hb.view(1, 3, 1))
    assert_sums_exact(torch.einsum("bcp,lc->blp", x.reshape(PATTERNS, C, P2), hw.abs()) + hb.abs().view(1, 3, 1), 0.125, BITS_INT, where)
    want = ref.float().to(fmt.dtype)[idx]
    ps, vs = ((2 * P2 + 15) // 16 * 16, (P2 + 15) // 16 * 16) if strided else (2 * P2, P2)
    fill = torch.tensor(-3.0, dtype=fmt.dtype)
    pol, val = torch.full((boards, ps), -3.0, dtype=fmt.dtype, device=device), torch.full((boards, vs), -3.0, dtype=fmt.dtype, device=device)
    xt = to_tiled(dll, x[idx], fmt, device)
    head = dll.azsp_head_tiled_f16 if fmt.f16 else dll.azsp_head_tiled
    hwd, hbd = hw.float().to(device), hb.float().to(device)
    assert head(xt.data_ptr(), hwd.data_ptr(), hbd.data_ptr(), pol.data_ptr(), val.data_ptr(), boards, S, C, 2, 1,
                ps if strided else 0, vs if strided else 0, None) == 0
    _sync(device)
    pol, val = pol.cpu(), val.cpu()
    assert_same_rows(pol[:, : 2 * P2], want[:, :2].reshape(boards, -1), where + " policy planes")
    assert_same_rows(val[:, :P2], want[:, 2].reshape(boards, -1), where + " value plane")
    assert bool((pol[:, 2 * P2:] == fill).all()) and bool((val[:, P2:] == fill).all()), where + ": padding columns were written"


# ---------------------------------------------------------------------------------------------------
# azsp_bias_act
# ---------------------------------------------------------------------------------------------------
def bias_act_exact(bnd, device, rows, channels, dtype, res, relu, seed=15):
    """azsp_bias_act on integers: y + bias (+ residual) is exact in fp32 and is rounded once, to nearest even, into the element type."""
    code, top, fmt = {torch.float32: (1, 2 ** 19, None), torch.bfloat16: (2, 256, BF16), torch.float16: (3, 2048, F16)}[dtype]
    g = torch.Generator().manual_seed(seed + channels)
    y = (1 if fmt is None else 8) * torch.randint(-top // 8, top, (rows, channels), generator=g).double()  # leans positive: the ReLU leaves enough to round
    b = torch.randint(-top, top + 1, (channels,), generator=g).double()
    r = torch.randint(-top, top + 1, (rows, channels), generator=g).double() if res else None
    where = f"bias_act {dtype} rows={rows} channels={channels} res={res} relu={relu}"
    assert_sums_exact(y.abs() + b.abs() + (r.abs() if res else 0), 1.0, 24, where)
    ref = y + b + (r if res else 0)
    ref = torch.relu(ref) if relu else ref
    if fmt is not None and rows * channels >= 1024:
        assert_rounding_is_tested(ref, fmt, where)
    yd, bd = y.to(dtype).to(device), b.to(dtype).to(device)
    rd = r.to(dtype).to(device) if res else None
    for t, s in ((yd, y), (bd, b)) + (((rd, r),) if res else ()):
        assert torch.equal(t.cpu().double(), s)
    assert bnd.dll.azsp_bias_act(yd.data_ptr(), bd.data_ptr(), rd.data_ptr() if res else None, rows, channels, code, relu, None) == 0
    _sync(device)
    assert_same_rows(yd.cpu(), ref.float().to(dtype), where)


# ---------------------------------------------------------------------------------------------------
# fully connected heads of the bf16 / f16 evaluator, and what holds for every head
# ---------------------------------------------------------------------------------------------------
PRIOR_REL = 4e-6   # |p - p64| <= PRIOR_REL * p64 per action: the exponent argument is exact, __expf scales it by log2(e) with one rounding
#                    (2^-24 * 12 * 1.44 * ln 2 = 7e-7 at a spread of 12), a few ulp for exp, the sum and the division: a margin of about 3
VALUE_ABS = 1e-6   # 16 ulp at 1
SUM_ABS = 1e-6
SPREAD = 12.0


def assert_heads(pri, val, logits64, pre64, where):
    """priors / values of a head kernel against fp64 on EXACT logits and value pre-activations: relative per action, absolute per value,
    sum of priors; torch's own fp32 softmax error on the same logits is recorded beside the kernel's."""
    spread = float((logits64.max(1).values - logits64.min(1).values).max())
    assert spread <= SPREAD, f"{where}: logit spread {spread} > {SPREAD}: the generator is wrong"
    assert torch.equal(logits64.float().double(), logits64) and torch.equal(pre64.float().double(), pre64)
    p64, v64 = torch.softmax(logits64, -1), torch.tanh(pre64)
    rel = (pri.double() - p64).abs() / p64
    trel = float(((torch.softmax(logits64.float(), -1).double() - p64).abs() / p64).max())
    b, a = divmod(int(rel.argmax()), p64.shape[1])
    dv = (val.double() - v64).abs()
    ds = float((pri.double().sum(1) - 1).abs().max())
    print(f"{where}: prior rel err {float(rel.max()):.3g} (board {b}, action {a}, p64 {float(p64[b, a]):.3g}; torch fp32 softmax {trel:.3g}; "
          f"smallest prior {float(p64.min()):.3g}), value err {float(dv.max()):.3g} (board {int(dv.argmax())}), |sum - 1| {ds:.3g}")
    assert float(rel.max()) <= PRIOR_REL, f"{where}: prior of board {b}, action {a}: {float(pri[b, a])!r} vs {float(p64[b, a])!r}, relative {float(rel.max()):.3g}"
    assert float(dv.max()) <= VALUE_ABS, f"{where}: value of board {int(dv.argmax())}: {float(dv.max()):.3g}"
    assert ds <= SUM_ABS, f"{where}: priors sum to 1 +- {ds:.3g}"


@functools.lru_cache(maxsize=None)
def fc_operands(P2, A, Fw, seed, rows=PATTERNS):
    """Head planes in 0..4 (half zero), sparse fully connected weights that are multiples of 1/16, biases that are multiples of 1/8."""
    g = torch.Generator().manual_seed(seed)
    pol, val = _int_acts(g, (rows, 2 * P2), top=4), _int_acts(g, (rows, P2), top=4)

    def sparse16(shape, density, top):
        w = torch.randint(1, top + 1, shape, generator=g).double() * (torch.randint(0, 2, shape, generator=g) * 2 - 1) / 16
        return torch.where(torch.rand(shape, generator=g) < density, w, torch.zeros((), dtype=torch.float64))

    wp, bp = sparse16((A, 2 * P2), 40.0 / (2 * P2), 2), torch.randint(-8, 9, (A,), generator=g).double() / 8
    w1, b1 = sparse16((Fw, P2), 20.0 / P2, 2), torch.randint(-8, 9, (Fw,), generator=g).double() / 8
    w2, b2 = sparse16((Fw,), 0.5, 4), 0.125
    return pol, val, wp, bp, w1, b1, w2, b2


def fc_heads_exact(bnd, device, P2, A, Fw, boards, fmt, seed=16):
    """azsp_fc_heads[_f16] on dyadic operands: every logit and the value pre-activation are exact, so what remains is exp, the sum, the
    division and tanh."""
    pol, val, wp, bp, w1, b1, w2, b2 = fc_operands(P2, A, Fw, seed)
    idx = pattern_index(boards)
    where = f"fc_heads {fmt.name} P2={P2} A={A} F={Fw} boards={boards}"
    logits = pol @ wp.T + bp
    hid = torch.relu(val @ w1.T + b1)
    pre = hid @ w2 + b2
    assert_sums_exact(pol @ wp.abs().T + bp.abs(), 1 / 16, BITS_INT, where + " logits")
    assert_sums_exact(val @ w1.abs().T + b1.abs(), 1 / 16, BITS_INT, where + " hidden")
    assert_sums_exact(hid @ w2.abs() + abs(b2), 1 / 256, BITS_INT, where + " value")
    k1, k2 = (2 * P2 + 15) // 16 * 16, (P2 + 15) // 16 * 16

    def padw(w, k):
        o = torch.zeros((w.shape[0] + 31) // 32 * 32, k, dtype=torch.float64)
        o[: w.shape[0], : w.shape[1]] = w
        assert torch.equal(o.to(fmt.dtype).double(), o)
        return o.to(fmt.dtype).to(device)

    def padv(v):
        o = torch.zeros((v.numel() + 31) // 32 * 32)
        o[: v.numel()] = v.float()
        return o.to(device)

    pd, vd = torch.zeros(boards + 1, k1, dtype=fmt.dtype), torch.zeros(boards + 1, k2, dtype=fmt.dtype)
    pd[:boards, : 2 * P2], vd[:boards, :P2] = pol[idx].to(fmt.dtype), val[idx].to(fmt.dtype)
    keep = (pd.to(device), vd.to(device), padw(wp, k1), padv(bp), padw(w1, k2), padv(b1), padv(w2))
    pri, v = torch.empty(boards, A, device=device), torch.empty(boards, device=device)
    fc = bnd.dll.azsp_fc_heads_f16 if fmt.f16 else bnd.dll.azsp_fc_heads
    assert fc(keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr(), k1 // 16, keep[4].data_ptr(), keep[5].data_ptr(), k2 // 16,
              keep[6].data_ptr(), ctypes.c_float(b2), pri.data_ptr(), v.data_ptr(), boards, A, Fw, None) == 0
    _sync(device)
    assert_heads(pri.cpu(), v.cpu(), logits[idx], pre[idx], where)


# ---------------------------------------------------------------------------------------------------
# fp32-class (split-precision) kernels: integer operands and operands that carry lo halves
# ---------------------------------------------------------------------------------------------------
def split_parts(t):
    """(hi, lo) of the split format as fp64: hi = f16(v), lo = f16((v - hi) * 2048), the header's definition."""
    t32 = t.float()
    assert torch.equal(t32.double(), t.double())
    hi = t32.half()
    lo = ((t32 - hi.float()) * 2048.0).half()
    return hi.double(), lo.double()


def assert_split_representable(ref, what):
    """ref survives fp32 and the split format (hi + lo / 2048) unchanged: the kernel's output stage has nothing to round."""
    hi, lo = split_parts(ref)
    assert torch.equal(hi + lo / 2048.0, ref.double()), what + ": the exact result is not representable in the split format"
    assert float(ref.abs().max()) <= 65504.0


def _carry(g, shape, density, signed, lmax=3, amin=5):
    """a + l / 2048 with a in {0, +-amin..7} (non-zero with probability `density`) and integer l in -lmax..lmax, l = 0 where a = 0."""
    a = torch.randint(amin, 8, shape, generator=g).double()
    if signed:
        a = a * (torch.randint(0, 2, shape, generator=g) * 2 - 1)
    a = torch.where(torch.rand(shape, generator=g) < density, a, torch.zeros((), dtype=torch.float64))
    l = torch.randint(-lmax, lmax + 1, shape, generator=g).double()
    return a + torch.where(a != 0, l, torch.zeros((), dtype=torch.float64)) / 2048.0


@functools.lru_cache(maxsize=None)
def split_conv_operands(S, C, kind, seed):
    """x, r, w, b of one fp32-class convolution as fp64.  kind "ints": every lo plane zero.  kind "carry": a + l / 2048 as above, the
    activations and the residual non-negative, the residual 32..63 + l / 2048 or 0, weights of density 5 / C, bias a multiple of 1/8."""
    g = torch.Generator().manual_seed(seed)
    shape = (PATTERNS, C, S, S)
    if kind == "ints":
        x = _int_acts(g, shape)
        r = torch.randint(0, 17, shape, generator=g).double()
        w = _int_weights(g, (C, C, 3, 3), 2)
        b = torch.randint(-16, 17, (C,), generator=g).double()
        return x, r, w, b
    x = _carry(g, shape, 0.5, False)
    ra = torch.randint(32, 64, shape, generator=g).double() + torch.randint(-3, 4, shape, generator=g).double() / 2048.0
    r = torch.where(torch.rand(shape, generator=g) < 0.5, ra, torch.zeros((), dtype=torch.float64))
    w = _carry(g, (C, C, 3, 3), 5.0 / C, True)
    b = torch.randint(-32, 33, (C,), generator=g).double() / 8
    return x, r, w, b


def split_reference(x, r, w, b, relu, kind, where, pad=1, cross_share=0.5):
    """The header's arithmetic in fp64 over the split parts: conv(xh, wh) + (conv(xh, wl) + conv(xl, wh)) / 2048 + b + r, then ReLU -- with
    the preconditions that make it order-independent and its result representable, all on the tensors given."""
    xh, xl = split_parts(x)
    wh, wl = split_parts(w)
    bv = b.view(1, -1, 1, 1)
    worst = _conv64(x.abs(), w.abs(), pad) + bv.abs() + (r.abs() if r is not None else 0)
    if kind == "ints":
        assert_integers(where, x, w, b, r)
        assert not xl.any() and not wl.any() and (r is None or not split_parts(r)[1].any()), where + ": lo planes must be zero"
        assert_sums_exact(worst, 1.0, BITS_INT, where)
    else:
        assert_integers(where + " (hi planes)", xh, wh, split_parts(r)[0] if r is not None else None)
        assert xl.any() and wl.any(), where + ": both lo planes must be non-zero somewhere"
        assert_integers(where + " (bias in 1/8)", b * 8)
        assert 2048.0 * float(worst.max()) < CAP_CARRY, f"{where}: 2048 * worst-case sum = 2^{torch.log2(2048.0 * worst.max()).item():.2f} >= 2^22"
    cross = _conv64(xh, wl, pad) + _conv64(xl, wh, pad)
    ref = _conv64(xh, wh, pad) + cross / 2048.0 + bv + (r if r is not None else 0)
    if kind == "carry":
        full = _conv64(x, w, pad) + bv + (r if r is not None else 0)
        assert bool(((ref - full).abs() <= _conv64(xl.abs(), wl.abs(), pad) / 2.0 ** 22).all()), where + ": only the lo x lo product may be missing"
        assert float((cross != 0).double().mean()) >= cross_share, where + ": the cross terms are not exercised"
    ref = torch.relu(ref) if relu else ref
    assert_split_representable(ref, where)
    return ref


def split_conv_exact(bnd, device, S, C, boards, kind, res, relu, seed=21):
    """azsp_conv3x3_split == the exact reference, compared as joined fp32 over every element."""
    x, r, w, b = split_conv_operands(S, C, kind, seed)
    idx = pattern_index(boards)
    where = f"conv3x3_split {kind} S={S} C={C} boards={boards} res={res} relu={relu}"
    ref = _per_pattern(lambda u: split_reference(x[u], r[u] if res else None, w, b, relu, kind, where), idx, ("split_conv", S, C, kind, res, relu, seed))
    out = su.split_conv(bnd, x[idx].float(), r[idx].float() if res else None, w.float(), b.float(), relu, device)
    assert out.roundtrip == 0.0, where + ": the layout round trip of exact operands must be exact"
    assert_same_cells(out.y.double(), ref, where)
    return out


@functools.lru_cache(maxsize=None)
def split_block_operands(S, kind, seed):
    """x, [w1, w2], [b1, b2] of a 64-filter fp32-class ResNetBlock.  "ints": dense integer weights.  "carry": the intermediate must be a
    carry operand again (integer hi plane, small lo), or conv2's sums would need more than 24 bits: conv1 has ONE weight +-(6..7) + l / 2048 per output
    channel on activations 6..7 + l / 2048 with |l| <= 2, so an intermediate value is 0 or 36..49 + (|.| <= 28) / 2048 (half an f16 step at
    32..64 is 32 / 2048); conv2 has four carry weights per output channel, which keeps 2048 * worst below 2^22."""
    C = 64
    g = torch.Generator().manual_seed(seed)
    shape = (PATTERNS, C, S, S)
    if kind == "ints":
        x = _int_acts(g, shape)
        ws = [_int_weights(g, (C, C, 3, 3), 1, skew=0.02), _int_weights(g, (C, C, 3, 3), 1, skew=0.02)]
        bs = [torch.randint(-16, 17, (C,), generator=g).double() for _ in range(2)]
        return x, ws, bs
    x = _carry(g, shape, 0.5, False, lmax=2, amin=6)

    def few(per_cout, lmax, amin):
        w = torch.zeros(C, C * 9, dtype=torch.float64)
        for co in range(C):
            at = torch.randperm(C * 9, generator=g)[:per_cout]
            w[co, at] = _carry(g, (per_cout,), 1.0, True, lmax=lmax, amin=amin)
        return w.view(C, C, 3, 3)

    ws = [few(1, 2, 6), few(4, 3, 5)]
    bs = [torch.zeros(C, dtype=torch.float64), torch.randint(-32, 33, (C,), generator=g).double() / 8]
    return x, ws, bs


def split_resblock_exact(bnd, device, S, boards, kind, seed=22):
    """azsp_resblock_split (and, beside it, the two azsp_conv3x3_split launches it must equal) == the exact reference of the block; the
    intermediate is exactly representable by the precondition of conv1, and is an exact operand of conv2 by that of conv2."""
    C = 64
    x, ws, bs = split_block_operands(S, kind, seed)
    idx = pattern_index(boards)
    where = f"resblock_split {kind} S={S} boards={boards}"

    def reference(u):
        mid = split_reference(x[u], None, ws[0], bs[0], 1, kind, where + " conv1", cross_share=0.25)  # (a quarter: conv1 and conv2 are sparse, see the generator)
        if kind == "carry":
            assert float((mid != 0).double().mean()) >= 0.1 and split_parts(mid)[1].any(), where + ": the intermediate carries no lo half"
        return split_reference(mid, x[u], ws[1], bs[1], 1, kind, where + " conv2", cross_share=0.25)

    ref = _per_pattern(reference, idx, ("split_block", S, kind, seed))
    yf, y2, y = su.split_resblock(bnd, x[idx].float(), [w.float() for w in ws], [b.float() for b in bs], device)
    assert_same_cells(y.double(), ref, where)
    assert_same_cells(su.from_split(bnd.dll, y2, boards, S, C).double(), ref, where + " (two launches)")


@functools.lru_cache(maxsize=None)
def split_stem_operands(n, C, kind, seed, cin=17):
    """x [PATTERNS,cin,n,n], w [C,cin,3,3], b.  "carry": carry planes (dense weights: 9 cin terms are few enough).  "exact": 0 / 1 planes, the
    engine's feature encoding, and carry weights."""
    g = torch.Generator().manual_seed(seed)
    x = _carry(g, (PATTERNS, cin, n, n), 0.5, False) if kind == "carry" else (torch.rand(PATTERNS, cin, n, n, generator=g) > 0.6).double()
    w = _carry(g, (C, cin, 3, 3), 0.3 if kind == "carry" else 0.9, True)
    b = torch.randint(-32, 33, (C,), generator=g).double() / 8
    return x, w, b


def split_stem_exact(bnd, device, n, C, pad, boards, kind, relu=1, seed=23):
    """azsp_split_features + azsp_stem_split on carry planes (17 of the 32 channels), or azsp_stem_split_exact on 0 / 1 planes, where it
    must also equal azsp_stem_split word for word."""
    x, w, b = split_stem_operands(n, C, kind, seed)
    idx = pattern_index(boards)
    So = n + 2 * (pad - 1)
    where = f"stem_split {kind} board={n} C={C} pad={pad} boards={boards} relu={relu}"

    def reference(u):
        xh, xl = split_parts(x[u])
        wh, wl = split_parts(w)
        bv = b.view(1, -1, 1, 1)
        assert_integers(where + " (hi planes)", xh, wh, b * 8)
        assert wl.any() and (xl.any() if kind == "carry" else not xl.any())
        worst = _conv64(x[u].abs(), w.abs(), pad) + bv.abs()
        assert 2048.0 * float(worst.max()) < CAP_CARRY, f"{where}: 2048 * worst-case sum = 2^{torch.log2(2048.0 * worst.max()).item():.2f} >= 2^22"
        ref = _conv64(xh, wh, pad) + (_conv64(xh, wl, pad) + _conv64(xl, wh, pad)) / 2048.0 + bv
        ref = torch.relu(ref) if relu else ref
        assert_split_representable(ref, where)
        return ref

    ref = _per_pattern(reference, idx, ("split_stem", n, C, pad, kind, relu, seed))
    raw, y, rec = su.split_stem(bnd.dll, x[idx].float(), w.float(), b.float(), pad, exact=kind == "exact", relu=relu, device=device)
    assert rec[0] == 0, where + ": range events on in-range operands"
    assert_same_cells(y.double(), ref, where)
    if kind == "exact":
        raw2, y2, _ = su.split_stem(bnd.dll, x[idx].float(), w.float(), b.float(), pad, exact=False, relu=relu, device=device)
        su.assert_same_words(raw, raw2, boards, C, So, where + " vs azsp_stem_split", y, y2)


@functools.lru_cache(maxsize=None)
def head_split_operands(S, C, A, Fw, seed, npol=2):
    """Tower output: carry activations of density 1/8; 1x1 weights in 1/8 with four non-zero channels per plane; fully connected weights in
    1/16 with four inputs per output; biases in 1/8 -- sparse because a head plane is a multiple of 2^-14 and a logit of 2^-18, which leaves
    2^24 * 2^-18 = 64 for the worst-case sum of a logit."""
    g = torch.Generator().manual_seed(seed)
    P2 = S * S
    x = _carry(g, (PATTERNS, C, S, S), 0.125, False)

    def few(rows, cols, per_row, top, den):
        w = torch.zeros(rows, cols, dtype=torch.float64)
        for i in range(rows):
            at = torch.randperm(cols, generator=g)[:per_row]
            w[i, at] = torch.randint(1, top + 1, (per_row,), generator=g).double() * (torch.randint(0, 2, (per_row,), generator=g) * 2 - 1) / den
        return w

    hw, hb = few(3, C, 4, 4, 8), torch.randint(0, 5, (3,), generator=g).double() / 8
    wp, bp = few(A, npol * P2, 4, 2, 16), torch.randint(-8, 9, (A,), generator=g).double() / 8
    w1, b1 = few(Fw, (3 - npol) * P2, 4, 2, 16), torch.randint(-4, 5, (Fw,), generator=g).double() / 8
    w2, b2 = few(1, Fw, 8, 2, 16)[0], 0.125
    return x, hw, hb, wp, bp, w1, b1, w2, b2


def head_split_exact(bnd, device, S, C, A, Fw, boards, npol=2, seed=24):
    """azsp_head_split on dyadic operands under the 24-bit precondition at every stage: head planes, logits and the value pre-activation are
    exact in fp32 in any order of summation."""
    dll = bnd.dll
    x, hw, hb, wp, bp, w1, b1, w2, b2 = head_split_operands(S, C, A, Fw, seed, npol)
    idx = pattern_index(boards)
    P2 = S * S
    where = f"head_split S={S} C={C} A={A} F={Fw} boards={boards}"
    xh, xl = split_parts(x)
    assert_integers(where + " (hi plane)", xh)
    assert xl.any()
    xf = x.reshape(PATTERNS, C, P2)
    hp = torch.relu(torch.einsum("bcp,lc->blp", xf, hw) + hb.view(1, 3, 1))
    assert_sums_exact(torch.einsum("bcp,lc->blp", xf, hw.abs()) + hb.abs().view(1, 3, 1), min(quantum(x) * quantum(hw), quantum(hb)), 24, where + " head planes")
    pin, vin = hp[:, :npol].reshape(PATTERNS, -1), hp[:, npol:].reshape(PATTERNS, -1)
    logits, hid = pin @ wp.T + bp, torch.relu(vin @ w1.T + b1)
    pre = hid @ w2 + b2
    assert_sums_exact(pin @ wp.abs().T + bp.abs(), min(quantum(pin) * quantum(wp), quantum(bp)), 24, where + " logits")
    assert_sums_exact(vin @ w1.abs().T + b1.abs(), min(quantum(vin) * quantum(w1), quantum(b1)), 24, where + " hidden")
    assert_sums_exact(hid @ w2.abs() + abs(b2), min(quantum(hid) * quantum(w2), b2), 24, where + " value")
    assert float((hp > 0).double().mean()) >= 0.2 and float((hid > 0).double().mean()) >= 0.2, where + ": the heads are mostly switched off"
    xs = su.to_split(dll, x[idx].float(), device)
    f = lambda t: t.float().contiguous().to(device)
    keep = (f(hw), f(hb), f(wp.T), f(bp), f(w1.T), f(b1), f(w2))
    pri, v = torch.empty(boards, A, device=device), torch.empty(boards, device=device)
    assert dll.azsp_head_split(xs.data_ptr(), *(k.data_ptr() for k in keep), ctypes.c_float(b2), pri.data_ptr(), v.data_ptr(), boards, S, C, A, Fw, npol,
                               None) == 0
    _sync(device)
    assert_heads(pri.cpu(), v.cpu(), logits[idx], pre[idx], where)
