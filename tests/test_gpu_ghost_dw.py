"""ycx_ghost_dw, bit for bit, on exactly representable operands (the bar of tests/test_gpu_gconv.py, whose
operand builder, grids, input conditions and bit comparison are imported).

out[.., j] = x[.., j] (+ res[.., j]) and out[.., c + j] = act(bias[j] + depthwise 5x5 of x) (+ res[.., c + j]):
the reference is torch's float64 ``F.conv2d`` on the CPU and every stored element must be RNE(true value),
equal bit patterns, no tolerance; the first half without a residual must be the input's bits.

Operands: ``operands(dtype, 1, 5, 1, h, w)`` of the grouped file for C = 48 (K = 25: bf16 grid (7, 7), fp16
(7, 8), fp32 on the bf16 operands) and a second set with C = 8 built the same way. Maps 13 x 11, 3 x 2 (every
window crosses a border and is smaller than the halo) and 5 x 17, n = 2. The input slice sits at channel 8 of
a buffer 24 wider with NaN in its padding channels, the 2C-wide output slice at channel 16 of a buffer 24
wider with the sentinel in its padding channels, which must survive. The residual is drawn on the 1 / 1024
grid within +-4 and rounded to the element type, so the first half has something to round too.

Shares of outputs that need rounding and of exact ties are asserted per case from the float64 reference
alone (MIN_ROUNDED, MIN_TIES of the grouped file; tests/test_ghost_plan.py checks the table on the CPU)."""
import ctypes
import functools
import types

import pytest
import torch
import torch.nn.functional as F

from helpers import dyadic, elt_ulps, rne
from test_gpu_gconv import (B_MAX, B_STEP, DTYPES, EXTRA, GRID, IN_OFF, OUT_OFF, SENTINEL, SPAN, TDT, W_MAX, X_MAX,
                            apply_act, assert_bits, check_inputs, operands)

L = pytest.importorskip("ycx._lib")

MAPS = [(13, 11), (3, 2), (5, 17)]
CS = (48, 8)
ACTS = [(L.ACT_NONE, 0.0), (L.ACT_LEAKY, 0.125)]
RES_STEP, RES_MAX = 1 / 1024, 4.0


@functools.lru_cache(maxsize=None)
def gh_operands(dtype, C, h, w, seed=0, grid=None):
    """x_full [n][h][w][C + 24] float64 (the slice at channel 8), wt [C][1][5][5], b [C] and the exact
    pre-activation z [n][C][h][w] of the depthwise 5x5 / s1 / p2 conv. C = 48 on the default grid: the
    grouped file's own operands; otherwise built the same way. Shared, never modified."""
    if C == 48 and grid is None and seed == 0:
        return operands(dtype, 1, 5, 1, h, w)
    K, n = 25, 2
    lx, lw, xm, wm = grid or (GRID[L.DT_BF16 if dtype == L.DT_F32 else dtype][K] + (X_MAX, W_MAX))
    assert K * 2 ** lx * 2 ** lw < SPAN
    g = torch.Generator().manual_seed(1000 * seed + 31 * K + 7 + h + 100 * C)
    o = types.SimpleNamespace(dtype=dtype, cin_g=1, k=5, s=1, h=h, w=w, n=n, C=C, groups=C, ho=h, wo=w)
    o.x_full = torch.full((n, h, w, C + EXTRA), SENTINEL, dtype=torch.float64)
    o.x_full[..., IN_OFF:IN_OFF + C] = dyadic((n, h, w, C), -xm, xm, xm / 2 ** lx, g)
    o.wt = dyadic((C, 1, 5, 5), -wm, wm, wm / 2 ** lw, g)
    o.b = dyadic((C,), -B_MAX, B_MAX, B_STEP, g)
    for t in (o.x_full, o.wt):
        assert torch.equal(t.to(TDT[dtype]).double(), t)
    o.z = F.conv2d(o.x_full[..., IN_OFF:IN_OFF + C].permute(0, 3, 1, 2), o.wt, o.b, 1, 2, groups=C)
    return o


def x_slice(o):
    return o.x_full[..., IN_OFF:IN_OFF + o.C]


def residual_of(o, seed=0):
    """float64 [n][h][w][2C] on the 1 / 1024 grid within +-4, rounded to the element type (fp32: to bf16)."""
    g = torch.Generator().manual_seed(77 + 13 * o.C + o.h + 1000 * seed)
    r = dyadic((o.n, o.h, o.w, 2 * o.C), -RES_MAX, RES_MAX, RES_STEP, g)
    return rne(r, torch.bfloat16 if o.dtype == L.DT_F32 else TDT[o.dtype]).double()


def reference(o, act, slope, r=None):
    """float64 NHWC [n][h][w][2C]: both halves before the one rounding to the element type."""
    ref = torch.cat([x_slice(o), apply_act(o.z, act, slope).permute(0, 2, 3, 1)], 3)
    return ref if r is None else ref + r


def desc_of(o, act=L.ACT_NONE, slope=0.0, residual=False, inplace=False):
    d = L.ConvDesc()
    d.n, d.h, d.w, d.cin, d.ho, d.wo, d.cout, d.cout_pad = o.n, o.h, o.w, o.C, o.h, o.w, 2 * o.C, 2 * o.C
    if inplace:  # one buffer: the 2C-wide slice at channel 16, its first half the input
        d.in_c_off, d.in_c_stride, d.out_c_off, d.out_c_stride = OUT_OFF, 2 * o.C + EXTRA, OUT_OFF, 2 * o.C + EXTRA
    else:
        d.in_c_off, d.in_c_stride, d.out_c_off, d.out_c_stride = IN_OFF, o.C + EXTRA, OUT_OFF, 2 * o.C + EXTRA
    d.kh = d.kw = 5
    d.stride, d.pad, d.act, d.leaky_slope = 1, 2, act, slope
    d.dtype, d.out_layout, d.groups = o.dtype, L.OUT_NHWC, o.C
    if residual:
        d.res_c_off, d.res_c_stride = 8, 2 * o.C + 8
    return d


def launch(device, o, act=L.ACT_NONE, slope=0.0, residual=None, inplace=False):
    """One call through the C ABI; the raw output buffer. Out of place: the input's padding channels hold
    NaN, the output is SENTINEL-filled. In place: the buffer is SENTINEL-filled with the input in the
    first half of the slice."""
    tdt = TDT[o.dtype]
    d = desc_of(o, act, slope, residual is not None, inplace)
    wp = o.wt.permute(2, 3, 0, 1).contiguous().float()  # [5][5][C][1] fp32, the grouped kernel's packing
    y = torch.full((o.n, o.h, o.w, 2 * o.C + EXTRA), SENTINEL, dtype=tdt)
    rd = None
    if residual is not None:
        rfull = torch.full((o.n, o.h, o.w, 2 * o.C + 8), SENTINEL, dtype=torch.float64)
        rfull[..., 8:] = residual
        rd = rfull.to(tdt).to(device)
    if inplace:
        y[..., OUT_OFF:OUT_OFF + o.C] = x_slice(o).to(tdt)
        yd = y.to(device)
        xd = yd
    else:
        xf = o.x_full.clone()
        xf[..., :IN_OFF] = float('nan')
        xf[..., IN_OFF + o.C:] = float('nan')
        xd, yd = xf.to(tdt).to(device), y.to(device)
    wd, bd = wp.to(device), o.b.float().to(device)
    L.check(L.lib.ycx_ghost_dw(ctypes.byref(d), xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), yd.data_ptr(),
                               L.ptr(rd), L.stream_handle(device)), "ycx_ghost_dw")
    torch.cuda.synchronize()
    return yd.cpu()


def expected(ref_nhwc, tdt):
    """The whole output buffer: RNE(ref) in the 2C-wide slice, the sentinel outside it."""
    exp = torch.full((*ref_nhwc.shape[:3], ref_nhwc.shape[3] + EXTRA), SENTINEL, dtype=tdt)
    exp[..., OUT_OFF:OUT_OFF + ref_nhwc.shape[3]] = rne(ref_nhwc, tdt)
    return exp


def check_case(o, act, slope, r=None, share=True):
    """The input conditions of one case, per half, from the float64 reference alone; the reference."""
    tdt = TDT[o.dtype]
    ref = reference(o, act, slope, r)
    if share:
        check_inputs(ref[..., o.C:], tdt, "second half")
        if r is not None:
            check_inputs(ref[..., :o.C], tdt, "first half")
    elif tdt == torch.float32:
        assert torch.equal(ref.float().double(), ref)
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('C', CS)
@pytest.mark.parametrize('hw', MAPS)
def test_exact_ghost(device, hw, C, dtype):
    """Act none and leaky 0.125, out of place and in place, no residual: the first half is the input's bits
    (out of place: copied; in place: untouched), the second RNE(float64 conv)."""
    tdt = TDT[dtype]
    o = gh_operands(dtype, C, *hw)
    for act, slope in ACTS:
        what = f"{hw[0]}x{hw[1]} C{C} dtype {dtype} act {act}"
        exp = expected(check_case(o, act, slope), tdt)
        assert_bits(exp[..., OUT_OFF:OUT_OFF + C].contiguous(), x_slice(o).to(tdt).contiguous(), "reference")
        assert_bits(launch(device, o, act, slope), exp, what + " out of place")
        assert_bits(launch(device, o, act, slope, inplace=True), exp, what + " in place")


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('C', CS)
@pytest.mark.parametrize('hw', MAPS)
def test_exact_ghost_residual(device, hw, C, dtype):
    """The shortcut over all 2C channels: x + r and act(acc + bias) + r, each rounded once."""
    tdt = TDT[dtype]
    o = gh_operands(dtype, C, *hw)
    r = residual_of(o)
    for act, slope in ACTS:
        what = f"residual {hw[0]}x{hw[1]} C{C} dtype {dtype} act {act}"
        ref = check_case(o, act, slope, r)
        assert_bits(launch(device, o, act, slope, residual=r), expected(ref, tdt), what)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES)
def test_exact_ghost_one_pixel(device, dtype):
    """A 1 x 1 map (every tap but the centre is outside the image), bits only: the sample is too small
    for the share assertion."""
    tdt = TDT[dtype]
    o = gh_operands(dtype, 48, 1, 1)
    r = residual_of(o)
    for act, slope in ACTS:
        exp = expected(check_case(o, act, slope, share=False), tdt)
        assert_bits(launch(device, o, act, slope), exp, "1x1 out of place")
        assert_bits(launch(device, o, act, slope, inplace=True), exp, "1x1 in place")
        assert_bits(launch(device, o, act, slope, residual=r),
                    expected(check_case(o, act, slope, r, share=False), tdt), "1x1 residual")


def grouped_second_half(device, o, xq, wq, bq, act):
    """ycx_conv2d_grouped (the generic kernel) on the same operands, writing the second half of the frame."""
    tdt = TDT[o.dtype]
    d = desc_of(o, act)
    d.cout = d.cout_pad = o.C
    d.out_c_off = OUT_OFF + o.C
    y = torch.full((o.n, o.h, o.w, 2 * o.C + EXTRA), SENTINEL, dtype=tdt).to(device)
    L.check(L.lib.ycx_conv2d_grouped(ctypes.byref(d), xq.data_ptr(), wq.data_ptr(), bq.data_ptr(), y.data_ptr(), None,
                                     L.stream_handle(device)), "ycx_conv2d_grouped")
    torch.cuda.synchronize()
    return y.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES)
def test_second_half_equals_the_grouped_kernel(device, dtype):
    """General operands (seeded normal x, w, b rounded to the element type; SiLU; 13 x 11 x 48): the fp32 sums
    are not exact, so this pins the accumulation order -- the second half equals ycx_conv2d_grouped's
    output bit for bit."""
    tdt = TDT[dtype]
    g = torch.Generator().manual_seed(5)
    o = types.SimpleNamespace(dtype=dtype, n=2, h=13, w=11, C=48)
    xf = torch.randn((o.n, o.h, o.w, o.C + EXTRA), generator=g).to(tdt)
    wq = torch.randn((5, 5, o.C, 1), generator=g).to(tdt).float().to(device)
    bq = torch.randn((o.C,), generator=g).to(tdt).float().to(device)
    xq = xf.to(device)
    d = desc_of(o, L.ACT_SILU)
    y = torch.full((o.n, o.h, o.w, 2 * o.C + EXTRA), SENTINEL, dtype=tdt).to(device)
    L.check(L.lib.ycx_ghost_dw(ctypes.byref(d), xq.data_ptr(), wq.data_ptr(), bq.data_ptr(), y.data_ptr(), None,
                               L.stream_handle(device)), "ycx_ghost_dw")
    torch.cuda.synchronize()
    got, par = y.cpu(), grouped_second_half(device, o, xq, wq, bq, L.ACT_SILU)
    lo = OUT_OFF + o.C
    assert torch.isfinite(par[..., lo:lo + o.C].float()).all()
    assert_bits(got[..., lo:].contiguous(), par[..., lo:].contiguous(), f"dtype {dtype}: second half vs grouped kernel")
    assert_bits(got[..., OUT_OFF:lo].contiguous(), xf[..., IN_OFF:IN_OFF + o.C].contiguous(), "first half")
    assert torch.equal(got[..., :OUT_OFF], torch.full_like(got[..., :OUT_OFF], SENTINEL))


def silu_operands(dtype):
    """As the grouped file's: z of a few units -- x in 1/8 steps of its half-range 2 (K = 25), w in 1/8 steps
    within +-1."""
    return gh_operands(dtype, 48, 13, 11, seed=3, grid=(3, 3, 2.0, 1.0))


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES)
def test_ghost_silu_ulps(device, dtype):
    """Plain YCX_ACT_SILU at the bar of test_gpu_gconv.test_grouped_silu_ulps (16-bit: check_silu; fp32: at
    most 4 ulps of the IEEE-division reference); the first half is still the input's bits."""
    from test_gpu_conv_exact import SILU_MAX_Z, check_silu
    tdt = TDT[dtype]
    o = silu_operands(dtype)
    assert float(o.z.abs().max()) <= SILU_MAX_Z
    got = launch(device, o, L.ACT_SILU, 0.0)
    lo = OUT_OFF + o.C
    assert_bits(got[..., OUT_OFF:lo].contiguous(), x_slice(o).to(tdt).contiguous(), "first half")
    half = got.clone()
    half[..., OUT_OFF:lo] = SENTINEL  # the frame check of check_silu: the sentinel everywhere but the second half
    if tdt == torch.float32:
        assert torch.equal(half[..., :lo], torch.full_like(half[..., :lo], SENTINEL))
        assert torch.equal(half[..., lo + o.C:], torch.full_like(half[..., lo + o.C:], SENTINEL))
        zz = o.z.permute(0, 2, 3, 1)
        ulps = elt_ulps(got[..., lo:lo + o.C].contiguous(), rne(zz / (1 + torch.exp(-zz)), tdt), tdt).abs()
        print(f"\nfp32 ghost SiLU: max {int(ulps.max())} ulps")
        assert int(ulps.max()) <= 4
    else:
        check_silu(half, o.z, L.ACT_SILU, tdt, f"ghost SiLU dtype {dtype}", lead=lo, tail=EXTRA - OUT_OFF)
