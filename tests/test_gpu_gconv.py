"""ycx_conv2d_grouped, bit for bit, on exactly representable operands (the exact-operand bar of
tests/test_gpu_conv_exact.py).

Operands and bias are dyadic rationals, so every fp32 product and partial sum is exact whatever the
order; the reference is torch's float64 ``F.conv2d(groups=...)`` on the CPU and the stored element
must be RNE(true sum) (helpers.rne): equality of bit patterns, no tolerance.

Grid: cin_g in {1, 2, 4, 8, 16} x k in {3, 5, 7} x s in {1, 2} x {bf16, fp16, f32}; n 2 on a 13 x 11
map (odd, no tile multiple), stride 2 also on 12 x 16; 48 channels (64 for cin_g 16: C % 16 == 0),
i.e. one full 32-channel chunk and a ragged one; the input slice at offset 8 of a buffer 24 wider,
the output slice at offset 16 of a buffer 24 wider, the padding channels holding a sentinel that
must survive. Act none and leaky 0.125 everywhere, a residual on a subset, SiLU on one case per
dtype at the ulp bar of test_gpu_conv_exact.test_silu_ulps (its check_silu, imported).

K = k * k * cin_g is small (9 .. 784), so the operand grids are chosen per (element type, K):
x in steps of 4 / 2^lx within +-4, w in steps of 2 / 2^lw within +-2 with (lx, lw) = GRID[...] below,
the pairs for which -- from the float64 reference alone -- at least 10 % of the outputs are not
representable in the element type and at least 1 % are exact ties (asserted per case, as in the dense
file), under the span bound K * 2^lx * 2^lw < 2^20 (asserted). fp32 outputs hold every sum exactly.
Both conditions are functions of the CPU reference only (tests/test_grouped_plan.py checks the whole
table without a GPU)."""
import ctypes
import functools
import math
import types

import pytest
import torch
import torch.nn.functional as F

from helpers import dyadic, elt_ulps, rne, rounding_stats

L = pytest.importorskip("ycx._lib")

TDT = {L.DT_BF16: torch.bfloat16, L.DT_F16: torch.float16, L.DT_F32: torch.float32}
SPAN = 1 << 20
MIN_ROUNDED, MIN_TIES = 0.10, 0.01
X_MAX, W_MAX, B_MAX, B_STEP = 4.0, 2.0, 2.0, 1 / 16
SENTINEL = 3.0  # representable in every element type
IN_OFF, OUT_OFF, EXTRA = 8, 16, 24
CIN_GS, KS, STRIDES = (1, 2, 4, 8, 16), (3, 5, 7), (1, 2)
DTYPES = [L.DT_BF16, L.DT_F16, L.DT_F32]
ACTS = [(L.ACT_NONE, 0.0), (L.ACT_LEAKY, 0.125)]

# (lx, lw) per (16-bit element type, K = k * k * cin_g); fp32 runs the bf16 operands
GRID = {
    L.DT_BF16: {9: (7, 7), 18: (7, 7), 36: (7, 7), 72: (6, 7), 144: (6, 6), 25: (7, 7), 50: (7, 7), 100: (6, 7),
                200: (6, 6), 400: (5, 6), 49: (7, 7), 98: (6, 7), 196: (6, 6), 392: (5, 6), 784: (5, 5)},
    L.DT_F16: {9: (8, 8), 18: (7, 8), 36: (7, 7), 72: (6, 7), 144: (6, 6), 25: (7, 8), 50: (7, 7), 100: (6, 7),
               200: (6, 6), 400: (5, 6), 49: (7, 7), 98: (6, 7), 196: (6, 6), 392: (5, 6), 784: (5, 5)},
}  # the finest grid under the span bound that the element type holds (bf16: 7 bits a side)


def channels(cin_g):
    return 64 if cin_g == 16 else 48


def maps(s):
    return [(13, 11)] + ([(12, 16)] if s == 2 else [])


@functools.lru_cache(maxsize=None)
def operands(dtype, cin_g, k, s, h, w, seed=0, grid=None):
    """Operands of one grouped conv (shared by every act / variant that runs it; never modified):
    x_full [n][h][w][C + 24] NHWC float64 (the slice at channel 8, SENTINEL around it), wt
    [C][cin_g][k][k], b [C] and the exact pre-activation z [n][C][ho][wo]. CPU only."""
    K, C, n = k * k * cin_g, channels(cin_g), 2
    lx, lw, xm, wm = grid or (GRID[L.DT_BF16 if dtype == L.DT_F32 else dtype][K] + (X_MAX, W_MAX))
    assert K * 2 ** lx * 2 ** lw < SPAN  # K * max|x|/step_x * max|w|/step_w
    sx, sw = xm / 2 ** lx, wm / 2 ** lw
    g = torch.Generator().manual_seed(1000 * seed + 31 * K + 7 * s + h)
    o = types.SimpleNamespace(dtype=dtype, cin_g=cin_g, k=k, s=s, h=h, w=w, n=n, C=C, groups=C // cin_g)
    o.x_full = torch.full((n, h, w, C + EXTRA), SENTINEL, dtype=torch.float64)
    o.x_full[..., IN_OFF:IN_OFF + C] = dyadic((n, h, w, C), -xm, xm, sx, g)
    o.wt = dyadic((C, cin_g, k, k), -wm, wm, sw, g)
    o.b = dyadic((C,), -B_MAX, B_MAX, B_STEP, g)
    tdt = TDT[dtype]
    for t in (o.x_full, o.wt):  # the element type holds the operands exactly
        assert torch.equal(t.to(tdt).double(), t)
    o.z = F.conv2d(o.x_full[..., IN_OFF:IN_OFF + C].permute(0, 3, 1, 2), o.wt, o.b, s, k // 2, groups=o.groups)
    o.ho, o.wo = o.z.shape[2:]
    return o


def apply_act(z, act, slope):
    return torch.where(z > 0, z, z * slope) if act == L.ACT_LEAKY else z


def check_inputs(ref64, tdt, what=""):
    """The input conditions of a case, from the float64 reference alone."""
    if tdt == torch.float32:
        assert torch.equal(ref64.float().double(), ref64), "fp32 does not hold the exact sums"
        return None
    rounded, ties = rounding_stats(ref64, tdt)
    assert rounded >= MIN_ROUNDED and ties >= MIN_TIES, \
        f"{what}: inputs too easy, {rounded:.3f} of the outputs need rounding, {ties:.3f} are ties"
    return rounded, ties


def desc_of(o, act=L.ACT_NONE, slope=0.0, residual=False):
    d = L.ConvDesc()
    d.n, d.h, d.w, d.cin, d.in_c_off, d.in_c_stride = o.n, o.h, o.w, o.C, IN_OFF, o.C + EXTRA
    d.ho, d.wo, d.cout, d.cout_pad, d.out_c_off, d.out_c_stride = o.ho, o.wo, o.C, o.C, OUT_OFF, o.C + EXTRA
    d.kh = d.kw = o.k
    d.stride, d.pad, d.act, d.leaky_slope = o.s, o.k // 2, act, slope
    d.dtype, d.out_layout, d.groups = o.dtype, L.OUT_NHWC, o.groups
    if residual:
        d.res_c_off, d.res_c_stride = 8, o.C + 8
    return d


def launch(device, o, act=L.ACT_NONE, slope=0.0, residual=None):
    """One grouped conv through the C ABI; the raw output buffer (SENTINEL-filled before the launch).
    residual: float64 [n][ho][wo][C], passed as the slice at channel 8 of a buffer 8 wider."""
    tdt = TDT[o.dtype]
    d = desc_of(o, act, slope, residual is not None)
    wp = o.wt.permute(2, 3, 0, 1).contiguous().float()  # [kh][kw][cout][cin_g] fp32 (include/ycx.h)
    y = torch.full((o.n, o.ho, o.wo, o.C + EXTRA), SENTINEL, dtype=tdt)
    rd = None
    if residual is not None:
        rfull = torch.full((o.n, o.ho, o.wo, o.C + 8), SENTINEL, dtype=torch.float64)
        rfull[..., 8:] = residual
        rd = rfull.to(tdt).to(device)
    xd, wd, bd, yd = o.x_full.to(tdt).to(device), wp.to(device), o.b.float().to(device), y.to(device)
    L.check(L.lib.ycx_conv2d_grouped(ctypes.byref(d), xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), yd.data_ptr(),
                                     L.ptr(rd), L.stream_handle(device)), "ycx_conv2d_grouped")
    torch.cuda.synchronize()
    return yd.cpu()


def expected(ref64, tdt):
    """The whole output buffer: RNE(ref) in the channel slice, the sentinel outside it."""
    r = ref64.permute(0, 2, 3, 1)
    exp = torch.full((*r.shape[:3], r.shape[3] + EXTRA), SENTINEL, dtype=tdt)
    exp[..., OUT_OFF:OUT_OFF + r.shape[3]] = rne(r, tdt)
    return exp


def assert_bits(got, exp, what=""):
    it = torch.int32 if got.dtype == torch.float32 else torch.int16
    assert got.shape == exp.shape and got.dtype == exp.dtype
    if torch.equal(got.contiguous().view(it), exp.contiguous().view(it)):
        return
    bad = got.contiguous().view(it) != exp.contiguous().view(it)
    dist = elt_ulps(got, exp, got.dtype)[bad]
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from RNE(true sum) (or the "
                         f"sentinel); distance in representable values: min {int(dist.min())}, max "
                         f"{int(dist.max())}; first at {[int(v) for v in bad.nonzero()[0]]}")


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('s', STRIDES)
@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('cin_g', CIN_GS)
def test_exact_grouped(device, cin_g, k, s, dtype):
    """The full grid, act none and leaky 0.125: borders, ragged tiles, a ragged channel chunk, both slices."""
    tdt = TDT[dtype]
    for h, w in maps(s):
        o = operands(dtype, cin_g, k, s, h, w)
        for act, slope in ACTS:
            what = f"cin_g {cin_g} k{k} s{s} {h}x{w} dtype {dtype} act {act}"
            ref = apply_act(o.z, act, slope)
            check_inputs(ref, tdt, what)
            assert_bits(launch(device, o, act, slope), expected(ref, tdt), what)


RES_CASES = [(1, 3, 1), (1, 7, 2), (2, 5, 1), (4, 3, 2), (8, 3, 1), (16, 3, 1), (16, 7, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('cin_g,k,s', RES_CASES)
def test_exact_grouped_residual(device, cin_g, k, s, dtype):
    """act(acc + bias) + residual: the residual on the 1/16 grid, the fp32 add exact, one rounding."""
    tdt = TDT[dtype]
    o = operands(dtype, cin_g, k, s, 13, 11)
    r = dyadic((o.n, o.ho, o.wo, o.C), -4, 4, 1 / 16, torch.Generator().manual_seed(cin_g * k + s))
    ref = apply_act(o.z, L.ACT_LEAKY, 0.125) + r.permute(0, 3, 1, 2)
    what = f"residual cin_g {cin_g} k{k} s{s} dtype {dtype}"
    check_inputs(ref, tdt, what)
    assert_bits(launch(device, o, L.ACT_LEAKY, 0.125, residual=r), expected(ref, tdt), what)


def silu_operands(dtype, cin_g, k, s):
    """As test_gpu_conv_exact.silu_operands: z of a few units -- x in steps of 1/8 of its half-range
    hx = min(4, 2^floor(log2(12 / sqrt(K)))), w in 1/8 steps within +-1: K * 8 * 8 < 2^20."""
    hx = min(4.0, 2.0 ** math.floor(math.log2(12 / math.sqrt(k * k * cin_g))))
    return operands(dtype, cin_g, k, s, 13, 11, seed=3, grid=(3, 3, hx, 1.0))


@pytest.mark.gpu
@pytest.mark.parametrize('dtype,cin_g,k,s', [(L.DT_BF16, 1, 3, 1), (L.DT_F16, 4, 5, 2), (L.DT_F32, 2, 3, 1)])
def test_grouped_silu_ulps(device, dtype, cin_g, k, s):
    """Plain YCX_ACT_SILU, one case per dtype. 16-bit: the bar of test_silu_ulps, its own check
    (bit-exact away from rounding boundaries, within one element-ulp everywhere). fp32 (the parity
    epilogue v / (1 + expf(-v)), IEEE division): expf within 1 ulp (2^-23 relative, and d silu / d e
    scales it by e / (1 + e) <= 1), the add and the division 2^-24 each: 2^-22 relative in all, at
    most 4 fp32 ulps of the result."""
    from test_gpu_conv_exact import SILU_MAX_Z, check_silu
    tdt = TDT[dtype]
    o = silu_operands(dtype, cin_g, k, s)
    zmax = float(o.z.abs().max())
    assert zmax <= SILU_MAX_Z, zmax
    got = launch(device, o, L.ACT_SILU, 0.0)
    assert torch.equal(got[..., :OUT_OFF], torch.full_like(got[..., :OUT_OFF], SENTINEL))
    assert torch.equal(got[..., OUT_OFF + o.C:], torch.full_like(got[..., OUT_OFF + o.C:], SENTINEL))
    body = got[..., OUT_OFF:OUT_OFF + o.C].contiguous()
    if tdt == torch.float32:
        zz = o.z.permute(0, 2, 3, 1)
        ref = zz / (1 + torch.exp(-zz))
        ulps = elt_ulps(body, rne(ref, tdt), tdt).abs()
        print(f"\nfp32 grouped SiLU: max {int(ulps.max())} ulps")
        assert int(ulps.max()) <= 4
    else:  # check_silu takes the raw buffer: this file's frame (slice at 16, 8 behind it) is the dense file's
        check_silu(got, o.z, L.ACT_SILU, tdt, f"grouped SiLU dtype {dtype} cin_g {cin_g} k{k} s{s}",
                   lead=OUT_OFF, tail=EXTRA - OUT_OFF)
