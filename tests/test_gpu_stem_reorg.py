"""ycx_stem_conv_reorg (ReOrg folded into the first conv) on exactly representable operands.

The exact-operand method of tests/test_gpu_conv_exact.py: image in 1/32 steps within +-4, weights in
1/32 steps within +-2 (both exact in bf16 and fp16), bias in 1/16 steps within +-2. K = 36 C <= 108
terms of at most 128 * 64 units of 2^-10: the span 108 * 128 * 64 = 884,736 < 2^20, so the fp32
accumulator holds the true sum whatever the K order and the stored element must be RNE(true sum).
The reference is torch's float64 conv2d over reorg(x), reorg being four strided slices and a cat
(nets/common.py:51). Every 16-bit case asserts from the reference alone that >= 10 % of its outputs
need rounding and >= 1 % are ties; the fp32 case that the cast is lossless.

Shapes (reorganised maps, n = 2): 9 x 11 (every border, a ragged pixel tail), 16 x 32, 8 x 64 (a full
MFMA row); stride 1 and 2; cout 32 and 64, 48 padded to 64; C = 3 and 1.

The frame of the exact files (tests/helpers.py): the output slice lies at channel 8 of a sentinel-filled
buffer 8 + cout + 8 wide, itself between sentinel guards, and whole buffers are compared; the fp32 image
lies between NaN guards of (2 * 2w + 2 + 1) floats (the 6x6 / pad-2 view of the conv) inside one
allocation; the padding rows of cout 48 in 64 are the operands' own channels 48 .. 63, not zeros.
tests/test_conv_exact_plan.py walks the tables below without a GPU."""
import ctypes
import functools
import types

import pytest
import torch
import torch.nn.functional as F

from helpers import (OUT_TAIL, SENTINEL, assert_bits, dyadic, elt_neighbours, elt_ulps, expected_frame, fetch_out,
                     guard_elems, guarded, guarded_out, out_frame, rne, rounding_stats)
from ycx import _lib as L  # a missing library is an error, on the CPU too (tests/test_conv_exact_plan.py)

gpu = pytest.mark.gpu  # every test here; the tables and builders import without a device

TDT = {L.DT_BF16: torch.bfloat16, L.DT_F16: torch.float16, L.DT_F32: torch.float32}
SPAN = 1 << 20
MIN_ROUNDED, MIN_TIES = 0.10, 0.01
ACTS = [(L.ACT_NONE, 0.0), (L.ACT_LEAKY, 0.125), (L.ACT_LEAKY, 0.25)]
X_MAX, X_STEP, W_MAX, W_STEP, B_MAX, B_STEP = 4.0, 1 / 32, 2.0, 1 / 32, 2.0, 1 / 16
OUT_EXTRA = 8  # the slice's channel offset; OUT_TAIL sentinel channels follow it
DTYPES = [L.DT_BF16, L.DT_F16, L.DT_F32]
COUTS = [32, 64]
BELOW_PAD = (48, 64)  # cout, cout_pad
SHAPES = [(9, 11), (16, 32), (8, 64)]
assert 108 * (X_MAX / X_STEP) * (W_MAX / W_STEP) == 884736 < SPAN


def reorg(x):
    return torch.cat([x[..., ::2, ::2], x[..., 1::2, ::2], x[..., ::2, 1::2], x[..., 1::2, 1::2]], 1)


@functools.lru_cache(maxsize=None)
def operands(h, w, s, c=3, grid=(X_STEP, W_STEP, X_MAX, W_MAX, B_MAX), seed=0):
    """Image [2][c][2h][2w], weights [64][4c][3][3], bias [64] (float64, never modified) and the exact
    pre-activation z of the conv over reorg(x), shared by every dtype / act / cout that runs it."""
    sx, sw, xm, wm, bm = grid
    assert 36 * c * (xm / sx) * (wm / sw) < SPAN
    g = torch.Generator().manual_seed(7919 * seed + 31 * h + w + 1000 * s + c)
    o = types.SimpleNamespace(n=2, h=h, w=w, s=s, c=c)
    o.x = dyadic((2, c, 2 * h, 2 * w), -xm, xm, sx, g)
    o.wt = dyadic((64, 4 * c, 3, 3), -wm, wm, sw, g)
    o.b = dyadic((64,), -bm, bm, B_STEP, g)
    for t in (o.x, o.wt):
        assert torch.equal(t.to(torch.bfloat16).double(), t) and torch.equal(t.to(torch.float16).double(), t)
    o.z = F.conv2d(reorg(o.x), o.wt, o.b, s, 1)
    o.ho, o.wo = o.z.shape[2:]
    return o


def apply_act(z, act, slope):
    return torch.where(z > 0, z, z * slope) if act == L.ACT_LEAKY else z


def check_inputs(ref64, tdt, what=""):
    if tdt == torch.float32:
        assert torch.equal(ref64.float().double(), ref64), "fp32 does not hold the exact sums"
        return
    rounded, ties = rounding_stats(ref64, tdt)
    assert rounded >= MIN_ROUNDED and ties >= MIN_TIES, \
        f"{what}: inputs too easy, {rounded:.3f} of the outputs need rounding, {ties:.3f} are ties"


def cpad_of(cout, dtype):
    return -(-cout // 64) * 64 if dtype == L.DT_F32 else (32 if cout <= 32 else -(-cout // 64) * 64)


def packed(o, cout, cpad):
    """fp32 weights [3][3][4C][cpad] and bias [cpad]: the padding channels cout .. cpad are the operands' own."""
    assert cpad <= o.wt.shape[0]
    assert cpad == cout or bool(o.wt[cout:cpad].flatten(1).any(1).all())  # no padding row is zero
    return o.wt[:cpad].permute(2, 3, 1, 0).contiguous().float(), o.b[:cpad].float()


def desc_of(o, dtype, cout, act=L.ACT_NONE, slope=0.0, cpad=None, out_scale=1.0):
    """The ycx_stem_conv_reorg descriptor of one case (no device)."""
    d = L.ConvDesc()
    d.n, d.h, d.w, d.cin, d.in_c_off, d.in_c_stride = o.n, o.h, o.w, 4 * o.c, 0, o.c
    d.ho, d.wo, d.cout, d.cout_pad = o.ho, o.wo, cout, cpad or cpad_of(cout, dtype)
    d.out_c_off, d.out_c_stride = OUT_EXTRA, OUT_EXTRA + cout + OUT_TAIL
    d.kh = d.kw = 3
    d.stride, d.pad, d.act, d.leaky_slope, d.dtype, d.out_layout = o.s, 1, act, slope, dtype, L.OUT_NHWC
    d.out_scale = out_scale
    return d


def image_guard(o):
    """Guard floats of the [n][C][2h][2w] image: the conv is a 6x6 / pad-2 conv over it (16-byte aligned
    behind the guard; the kernel asks for 8)."""
    return guard_elems(2, 2 * o.w, 1, 4)


E4M3 = torch.float8_e4m3fn
SENTINEL_BYTE = int(torch.tensor(SENTINEL).to(E4M3).view(torch.uint8))  # the e4m3 code of the sentinel


def launch(device, o, dtype, cout, act=L.ACT_NONE, slope=0.0, cpad=None, out_scale=1.0, via_ops=False):
    """One call through the C ABI (or as a YCX_OP_STEM_REORG through ycx_run_ops); the raw output buffer."""
    d = desc_of(o, dtype, cout, act, slope, cpad, out_scale)
    wp, bp = packed(o, cout, d.cout_pad)
    if dtype == L.DT_FP8:
        y, sentinel = torch.full((o.n, o.ho, o.wo, d.out_c_stride), SENTINEL_BYTE, dtype=torch.uint8), SENTINEL_BYTE
    else:
        y, sentinel = out_frame(o.n, o.ho, o.wo, cout, TDT[dtype], OUT_EXTRA), SENTINEL
    xd, wd, bd = guarded(o.x.float(), image_guard(o), device), wp.to(device), bp.to(device)
    yd = guarded_out(y, device)
    st = L.stream_handle(device)
    if via_ops:
        op = L.Op()
        op.kind = L.OP_STEM_REORG
        op.d.conv = d
        op.in_, op.weight, op.bias, op.out = xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), yd.data_ptr()
        L.check(L.lib.ycx_run_ops(ctypes.byref(op), 1, st, None), "ycx_run_ops")
    else:
        L.check(L.lib.ycx_stem_conv_reorg(ctypes.byref(d), xd.data_ptr(), wd.data_ptr(), bd.data_ptr(),
                                          yd.data_ptr(), st), "ycx_stem_conv_reorg")
    torch.cuda.synchronize()
    return fetch_out(yd, sentinel, what="stem_reorg")


def expected(ref64, tdt):
    """The whole output buffer: RNE(ref) in the channel slice, the sentinel outside it."""
    return expected_frame(rne(ref64.permute(0, 2, 3, 1), tdt), OUT_EXTRA)


def run_acts(device, o, dtype, cout, what, cpad=None):
    tdt = TDT[dtype]
    for act, slope in ACTS:
        ref = apply_act(o.z[:, :cout], act, slope)
        check_inputs(ref, tdt, what)
        got = launch(device, o, dtype, cout, act, slope, cpad=cpad)
        assert_bits(got, expected(ref, tdt), f"{what} act {act} slope {slope}")


@gpu
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('cout', COUTS)
@pytest.mark.parametrize('s', [1, 2])
@pytest.mark.parametrize('h,w', SHAPES)
def test_exact_stem_reorg(device, h, w, s, cout, dtype):
    run_acts(device, operands(h, w, s), dtype, cout, f"stem_reorg {h}x{w} s{s} cout {cout} dtype {dtype}")


@gpu
@pytest.mark.parametrize('dtype', DTYPES)
def test_exact_stem_reorg_cout_below_pad(device, dtype):
    """cout 48 in a 64-channel pad: channels 48..63 of the pad are computed on live rows and never stored."""
    cout, cpad = BELOW_PAD
    run_acts(device, operands(9, 11, 1), dtype, cout, f"stem_reorg cout {cout}/{cpad} dtype {dtype}", cpad=cpad)


@gpu
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('s', [1, 2])
def test_exact_stem_reorg_one_channel(device, s, dtype):
    """C = 1 (a grey image): 4 reorganised channels, K = 36 in two MFMA steps."""
    run_acts(device, operands(9, 11, s, c=1), dtype, 32, f"stem_reorg C1 s{s} dtype {dtype}")


@gpu
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('s', [1, 2])
def test_op_stem_reorg_matches_direct_call(device, s, dtype):
    o = operands(9, 11, s)
    a = launch(device, o, dtype, 64, L.ACT_LEAKY, 0.125)
    b = launch(device, o, dtype, 64, L.ACT_LEAKY, 0.125, via_ops=True)
    it = torch.int32 if dtype == L.DT_F32 else torch.int16
    assert torch.equal(a.view(it), b.view(it))
    assert_bits(a, expected(apply_act(o.z, L.ACT_LEAKY, 0.125), TDT[dtype]), "direct")


# ---- e4m3 store: bit-exact (tests/test_gpu_fp8_exact.py): the operands are exact, the fp32 value is cast
# straight to e4m3, so every byte is torch's cast of clamp(ref * out_scale, +-448) ----
FP8_CASES = [(9, 11, 64), (8, 64, 32)]


@gpu
@pytest.mark.parametrize('s', [1, 2])
@pytest.mark.parametrize('h,w,cout', FP8_CASES)
def test_stem_reorg_fp8_store(device, h, w, cout, s):
    o = operands(h, w, s)
    so = 4.0  # where |z| passes 112 the +-448 clamp is exercised too
    for act, slope in ACTS[:2]:
        ref = apply_act(o.z[:, :cout], act, slope).permute(0, 2, 3, 1)
        got = launch(device, o, L.DT_FP8, cout, act, slope, out_scale=so)
        exp = torch.full_like(got, SENTINEL_BYTE)
        exp[..., OUT_EXTRA:OUT_EXTRA + cout] = rne((ref * so).clamp(-448.0, 448.0), E4M3).view(torch.uint8)
        bad = got != exp
        assert not bad.any(), f"stem_reorg fp8 {h}x{w} s{s} act {act}: {int(bad.sum())} of {bad.numel()} bytes differ " \
                              f"from e4m3(clamp(ref * so)); first at {[int(v) for v in bad.nonzero()[0]]}"


# ---- SiLU and pre-scaled SiLU at ulp level: check_silu of tests/test_gpu_conv_exact.py restated ----
LOG2E = 1.4426950408889634
SILU_MAX_Z = 32.0
MAX_EXCUSED = {torch.bfloat16: 0.01, torch.float16: 0.05}


def silu_ref(z, act):
    if act == L.ACT_SILU_PS:  # z = -log2(e) c: c / (1 + 2^z)
        return (-z / LOG2E) / (1 + torch.exp2(z))
    return z / (1 + torch.exp(-z))


def silu_conditions(z, act, tdt, what):
    """The input conditions of a SiLU case, from the reference alone: the NHWC reference, the excused
    elements, the fp16 subnormal results."""
    assert float(z.abs().max()) <= SILU_MAX_Z, "input condition: |z| <= 32"
    zz = z.permute(0, 2, 3, 1).contiguous()
    ref = silu_ref(zz, act)
    lo, hi = elt_neighbours(ref, tdt)
    margin = (zz.abs() + 8) * 2.0 ** -23 * ref.abs()
    excused = (lo != hi) & ((ref - (lo + hi) / 2).abs() <= margin)
    sub = (ref.abs() < 2.0 ** -14) if tdt == torch.float16 else torch.zeros_like(excused)
    share = float((excused & ~sub).double().mean())
    assert share <= MAX_EXCUSED[tdt], f"{what}: input condition, {share:.4f} of the elements are excused"
    return ref, excused, sub, share


def check_silu(got, z, act, tdt, what):
    """Bit-exact where the float64 reference lies farther than (|z| + 8) 2^-23 relative from a rounding
    boundary, within one element-ulp of RNE(reference) everywhere (fp16 subnormals: 2^-24 absolute)."""
    ref, excused, sub, share = silu_conditions(z, act, tdt, what)
    c = ref.shape[3]
    frame = got.clone()
    frame[..., OUT_EXTRA:OUT_EXTRA + c] = SENTINEL
    assert_bits(frame, torch.full_like(got, SENTINEL), f"{what}: wrote outside the output channel slice")
    g = got[..., OUT_EXTRA:OUT_EXTRA + c].contiguous()
    ulps = elt_ulps(g, rne(ref, tdt), tdt)
    if sub.any():
        assert float((g.double() - ref).abs()[sub].max()) <= 2.0 ** -24, what
    assert int(ulps[~sub].abs().max()) <= 1, f"{what}: {int(ulps[~sub].abs().max())} element-ulps from RNE(ref)"
    must = ~excused & ~sub
    bad = must & (ulps != 0)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {int(must.sum())} elements away from a rounding " \
                          f"boundary differ from RNE(ref) ({share:.4f} excused, {int(sub.sum())} subnormal)"


SILU_GRID = (1 / 8, 1 / 8, 1.0, 1.0, 1.0)


@gpu
@pytest.mark.parametrize('act', [L.ACT_SILU, L.ACT_SILU_PS])
@pytest.mark.parametrize('dtype', [L.DT_BF16, L.DT_F16])
@pytest.mark.parametrize('s', [1, 2])
def test_silu_ulps_stem_reorg(device, s, dtype, act):
    """x and w in 1/8 steps within +-1 (K = 108: hx = 2^floor(log2(12 / sqrt(K))) = 1), bias in 1/16 steps
    within +-1: z of a few units. YCX_ACT_SILU_PS: the weights and bias themselves are on the grid."""
    o = operands(9, 11, s, grid=SILU_GRID, seed=3)
    got = launch(device, o, dtype, 64, act, 0.0)
    check_silu(got, o.z, act, TDT[dtype], f"stem_reorg s{s} dtype {dtype} act {act}")
