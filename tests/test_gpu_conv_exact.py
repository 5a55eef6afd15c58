"""Bit-exact conv parity on exactly representable operands ("exact-operand bar").

Operands and bias are small dyadic rationals, so every product and every partial sum is exactly
representable in fp32: the accumulator holds the true sum whatever the tile's K order, split-K
split or MFMA grouping, and the stored element must be RNE(true sum) bit for bit -- no tolerance.
The reference is torch's float64 conv on the CPU; the element reference is its cast (helpers.rne).

The frame (helpers.py, "the frame of the exact files"): every output is a whole sentinel-filled
buffer with the channel slice in its interior (NHWC: channel 16 of 16 + cout + 8, a lead of 8 for
the x2 store and the stems; fp32 NCHW: plane 1 of cout + 2) between two sentinel guards, compared
bit for bit over the whole buffer; every input slice lies at channel 8 of 8 + cin + 8 channels with
NaN around it, the residual likewise, and every input tensor (the stems' fp32 images included) lies
between NaN guards inside one allocation; wherever cout < cout_pad the padding weight rows and bias
entries hold grid values (the operands' own channels cout .. cout_pad), so a stored padding channel
is a value and not the 0 of a zero row. tests/test_conv_exact_plan.py walks the case tables below
without a GPU: span, lossless operands, rounded / tie shares, the live padding, the descriptors.

Grids (helpers.dyadic), chosen per case so that K * max|x|/step_x * max|w|/step_w < 2^20:
  base   x in 1/4 steps within +-4, w in 1/4 steps within +-2, bias in 1/16 steps within +-2
         (bf16 at every K, fp16 at K >= 2304, fp32)
  fine   x in 1/16 steps, w in 1/8 steps (fp16 at K <= 576: eleven significand bits need more
         low bits before anything has to be rounded); fp16 at 576 < K < 2304: the finest of
         (1/16, 1/8), (1/8, 1/8), (1/8, 1/4), (1/4, 1/4) under the 2^20 bound
Every 16-bit case asserts from the float64 reference alone that >= 10 % of its outputs are not
representable in the element type and >= 1 % are exact ties (conditions on the inputs; fp32
outputs hold every sum exactly, so there the condition is that the fp32 cast is lossless).

tile -> cases (each in bf16 and fp16; tile 8 in fp32):
  1-7, 9-18, 24-26, 56   test_exact_general_tiles: n 2, 13 x 11,
                         (k, s) in (1,1) (3,1) (3,2) (5,1); act none, leaky 0.125, leaky 0.25
  8                      test_exact_f32_tile8 (the same operands)
  19, 20, 21, 23         test_exact_special_kernels 16 x 16 and 32 x 48
  48, 49                 test_exact_special_kernels 40 x 40
  50                     test_exact_special_kernels 32 x 64 and 31 x 63
  22                     test_exact_special_kernels 13 x 11 (cin 64 / 256) and n 2, 96 x 96
  3, 7, 16, 18, 56, 20, 48   test_exact_epilogue_variants (residual, x2 upsample, fp32 NCHW, cout < cout_pad)
  16                     test_exact_up2_cout_below_pad (120 of 128 through the x2 store)
  22, 23, 49, 50         test_exact_cout_below_pad
  16, 18, 56             test_exact_splitk (k_split 2, 3, 4; tile 16's chunk-major stride-2 order)
  16                     test_exact_tile16_s2_cin128_chunk_major (unsplit)
  16, 18, 25             test_exact_fused_pool
  55                     test_exact_conv2d_pair
  38 (head)              test_exact_head_raw_store
  stem, stem2            test_exact_stem, test_exact_stem2
  3, 16, 18, 20, 22, 23, 50, split-K reduce, stem2   test_silu_ulps (SiLU and pre-scaled SiLU)
"""
import ctypes
import functools
import math
import types

import pytest
import torch
import torch.nn.functional as F

from helpers import (IN_LEAD, IN_TAIL, OUT_LEAD, OUT_TAIL, SENTINEL, SENTINEL_F32, assert_bits, dyadic, elt_neighbours,
                     elt_ulps, expected_frame, expected_planes, fetch_out, guard_elems, guarded, guarded_out,
                     live_padding_share, nan_frame, out_frame, out_planes, rne, rounding_stats)
from ycx import _lib as L  # a missing library is an error, on the CPU too (tests/test_conv_exact_plan.py)

gpu = pytest.mark.gpu  # every test here; the tables and builders import without a device

TDT = {L.DT_BF16: torch.bfloat16, L.DT_F16: torch.float16, L.DT_F32: torch.float32}
DT16 = [L.DT_BF16, L.DT_F16]
SPAN = 1 << 20                    # K * max|x|/step_x * max|w|/step_w stays below this
MIN_ROUNDED, MIN_TIES = 0.10, 0.01
ACTS = [(L.ACT_NONE, 0.0), (L.ACT_LEAKY, 0.125), (L.ACT_LEAKY, 0.25)]  # both slopes exact, neither is 0.1
X_MAX, W_MAX, B_MAX, B_STEP = 4.0, 2.0, 2.0, 1 / 16
_FP16_GRIDS = [(1 / 16, 1 / 8), (1 / 8, 1 / 8), (1 / 8, 1 / 4), (1 / 4, 1 / 4)]
UP2_LEAD = STEM_LEAD = 8          # the x2 store and the stems keep their slice at channel 8


def pick_grid(K, dtype):
    """(step_x, step_w) for a conv of K terms stored as ``dtype`` (module docstring)."""
    if dtype != L.DT_F16 or K >= 2304:
        sx, sw = 1 / 4, 1 / 4
    elif K <= 576:
        sx, sw = _FP16_GRIDS[0]
    else:
        sx, sw = next(g for g in _FP16_GRIDS if K * (X_MAX / g[0]) * (W_MAX / g[1]) < SPAN)
    assert K * (X_MAX / sx) * (W_MAX / sw) < SPAN, (K, sx, sw)
    return sx, sw


def apply_act(z, act, slope):
    return torch.where(z > 0, z, z * slope) if act == L.ACT_LEAKY else z


def check_inputs(ref64, tdt, what=""):
    """The input conditions of a 16-bit case, from the float64 reference alone."""
    if tdt == torch.float32:
        assert torch.equal(ref64.float().double(), ref64), "fp32 does not hold the exact sums"
        return None
    rounded, ties = rounding_stats(ref64, tdt)
    assert rounded >= MIN_ROUNDED and ties >= MIN_TIES, \
        f"{what}: inputs too easy, {rounded:.3f} of the outputs need rounding, {ties:.3f} are ties"
    return rounded, ties


@functools.lru_cache(maxsize=None)
def operands(dtype, n, h, w, cin, k, s, in_extra=IN_LEAD, pool=False, seed=0, grid=None, cout=256):
    """Operands of one conv (shared by every tile / act / variant that runs it; never modified):
    x_full [n][h][w][in_extra + cin + 8] NHWC float64 (the slice at channel in_extra, NaN around it),
    wt [cout][cin][k][k], b [cout] and the exact pre-activation z [n][cout][ho][wo]. pool: x_full is the
    (2h, 2w) map of the fused max-pool. grid: (step_x, step_w, max|x|, max|w|) where a case needs
    another than pick_grid's. CPU only."""
    sx, sw, xm, wm = grid or (pick_grid(cin * k * k, dtype) + (X_MAX, W_MAX))
    assert cin * k * k * (xm / sx) * (wm / sw) < SPAN
    g = torch.Generator().manual_seed(1000 * seed + 17 * cin + k + s)
    up = 2 if pool else 1
    o = types.SimpleNamespace(n=n, h=h, w=w, cin=cin, k=k, s=s, in_extra=in_extra, pool=pool, dtype=dtype,
                              grid=(sx, sw, xm, wm))
    xs = dyadic((n, up * h, up * w, in_extra + cin), -xm, xm, sx, g)[..., in_extra:]
    o.x_full = nan_frame(xs, in_extra, IN_TAIL)
    o.wt = dyadic((cout, cin, k, k), -wm, wm, sw, g)
    o.b = dyadic((cout,), -B_MAX, B_MAX, B_STEP, g)
    tdt = TDT[dtype]
    for t in (xs, o.wt):  # the element type holds the operands exactly
        assert torch.equal(t.to(tdt).double(), t)
    x = xs.permute(0, 3, 1, 2)
    if pool:
        x = F.max_pool2d(x, 2, 2)  # exact
    o.x = x
    o.z = F.conv2d(x, o.wt, o.b, s, k // 2)
    o.ho, o.wo = o.z.shape[2:]
    return o


def cpad_of(cout, dtype):
    if dtype == L.DT_F32:
        return -(-cout // 64) * 64
    return 32 if cout <= 32 else 64 if cout <= 64 else -(-cout // 128) * 128


def padding_rows(o, cout, cpad):
    """Weight rows [cpad - cout][cin][k][k] and bias [cpad - cout] of the padding channels: the operands' own
    channels cout .. cpad where ``operands`` drew that many, else fresh draws from the same grid."""
    if o.wt.shape[0] >= cpad:
        return o.wt[cout:cpad], o.b[cout:cpad]
    sx, sw, xm, wm = o.grid
    g = torch.Generator().manual_seed(77 + cout + 3 * cpad + o.cin)
    return (dyadic((cpad - cout, o.cin, o.k, o.k), -wm, wm, sw, g), dyadic((cpad - cout,), -B_MAX, B_MAX, B_STEP, g))


def packed(o, cout, cpad):
    """wp [cpad][k][k][cin] in the element type and the fp32 bias [cpad], padding rows live."""
    tdt = TDT[o.dtype]
    wt, b = o.wt[:cout], o.b[:cout]
    if cpad > cout:
        wx, bx = padding_rows(o, cout, cpad)
        assert bool(wx.flatten(1).any(1).all())  # no padding row is zero
        wt, b = torch.cat([wt, wx]), torch.cat([b, bx])
    wp = wt.permute(0, 2, 3, 1).contiguous().to(tdt)
    assert torch.equal(wp.double(), wt.permute(0, 2, 3, 1))
    return wp, b.float()


def padding_stores(o, cout, cpad, act, slope, out_dt):
    """What the padding channels cout .. cpad would store (element type ``out_dt``), from the reference."""
    wx, bx = padding_rows(o, cout, cpad)
    z = o.z[:, cout:cpad] if o.wt.shape[0] >= cpad else F.conv2d(o.x, wx, bx, o.s, o.k // 2)
    return rne(apply_act(z, act, slope), out_dt)


def check_live_padding(o, cout, cpad, act, slope, layout=L.OUT_NHWC):
    """The live-padding condition of one cout < cout_pad case (CPU only): >= 90 % of what the padding
    channels would store differs in its bits from the sentinel it would land on."""
    f32 = layout == L.OUT_NCHW_F32
    return live_padding_share(padding_stores(o, cout, cpad, act, slope, torch.float32 if f32 else TDT[o.dtype]),
                              SENTINEL_F32 if f32 else SENTINEL)


def conv_desc(o, tile, cout, act=L.ACT_NONE, slope=0.0, lead=OUT_LEAD, tail=OUT_TAIL, residual=False,
              layout=L.OUT_NHWC, k_split=0, cpad=None):
    """The ycx_conv2d descriptor of one case (no device)."""
    d = L.ConvDesc()
    d.n, d.h, d.w, d.cin, d.in_c_off, d.in_c_stride = o.n, o.h, o.w, o.cin, o.in_extra, o.x_full.shape[3]
    d.ho, d.wo, d.cout, d.cout_pad = o.ho, o.wo, cout, cpad or cpad_of(cout, o.dtype)
    d.out_c_off, d.out_c_stride = (1, cout + 2) if layout == L.OUT_NCHW_F32 else (lead, lead + cout + tail)
    d.kh = d.kw = o.k
    d.stride, d.pad, d.act, d.leaky_slope = o.s, 0 if o.pool else o.k // 2, act, slope
    d.dtype, d.out_layout, d.tile, d.k_split, d.in_pool = o.dtype, layout, tile, k_split, int(o.pool)
    if residual:
        d.res_c_off, d.res_c_stride = IN_LEAD, IN_LEAD + cout + IN_TAIL
    return d


def input_guard(d, itemsize):
    """Guard elements of the NHWC input of descriptor ``d`` (the (2h, 2w) map of a fused pool: pad 0)."""
    return guard_elems(d.pad, d.w * (2 if d.in_pool else 1), d.in_c_stride, itemsize)


def launch(device, o, tile, cout, act=L.ACT_NONE, slope=0.0, lead=OUT_LEAD, tail=OUT_TAIL, residual=None,
           layout=L.OUT_NHWC, k_split=0, cpad=None):
    """One conv through the C ABI on operands ``o`` (first ``cout`` channels); the raw output buffer.
    residual: float64 [n][ho][wo][cout], passed as the slice at channel 8 of a NaN-framed, guarded buffer."""
    tdt = TDT[o.dtype]
    d = conv_desc(o, tile, cout, act, slope, lead, tail, residual is not None, layout, k_split, cpad)
    wp, bp = packed(o, cout, d.cout_pad)
    up = 2 if layout == L.OUT_NHWC_UP2 else 1
    if layout == L.OUT_NCHW_F32:
        y, sentinel = out_planes(o.n, cout, o.ho, o.wo), SENTINEL_F32
    else:
        y, sentinel = out_frame(o.n, o.ho * up, o.wo * up, cout, tdt, lead, tail), SENTINEL
    xd = guarded(o.x_full.to(tdt), input_guard(d, tdt.itemsize), device)
    wd, bd, yd = wp.to(device), bp.to(device), guarded_out(y, device)
    rd = None
    if residual is not None:
        rd = guarded(nan_frame(residual).to(tdt), guard_elems(0, o.wo, d.res_c_stride, tdt.itemsize), device)
    st = L.stream_handle(device)
    if k_split > 1:
        nws = int(L.lib.ycx_conv_workspace_size(ctypes.byref(d)))
        assert nws == k_split * o.n * o.ho * o.wo * d.cout_pad * 4
        ws = torch.full((nws // 4,), float('nan'), device=device)  # every partial must be overwritten
        L.check(L.lib.ycx_conv2d_ws(ctypes.byref(d), xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), yd.data_ptr(),
                                    L.ptr(rd), ws.data_ptr(), nws, st))
    else:
        L.check(L.lib.ycx_conv2d(ctypes.byref(d), xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), yd.data_ptr(),
                                 L.ptr(rd), st))
    torch.cuda.synchronize()
    return fetch_out(yd, sentinel, what=f"tile {tile}")


def expected(ref64, tdt, layout=L.OUT_NHWC, lead=OUT_LEAD, tail=OUT_TAIL):
    """The whole output buffer: RNE(ref) in the channel slice, the sentinel outside it."""
    if layout == L.OUT_NCHW_F32:
        check_inputs(ref64, torch.float32)
        return expected_planes(ref64.float())
    r = ref64.permute(0, 2, 3, 1)
    if layout == L.OUT_NHWC_UP2:
        r = r.repeat_interleave(2, 1).repeat_interleave(2, 2)
    return expected_frame(rne(r, tdt), lead, tail)


def run_acts(device, o, tile, cout, what, **kw):
    """act none, leaky 0.125 and leaky 0.25 of one conv, each bit-exact."""
    tdt = TDT[o.dtype]
    for act, slope in ACTS:
        ref = apply_act(o.z[:, :cout], act, slope)
        check_inputs(ref, tdt, what)
        got = launch(device, o, tile, cout, act, slope, **kw)
        assert_bits(got, expected(ref, tdt), f"{what} act {act} slope {slope}")


# tile -> (cout, cin) of the general cases (cout = the tile's channel width, cin its K step or twice it)
GENERAL = {1: (128, 64), 2: (64, 64), 3: (64, 64), 4: (128, 64), 5: (32, 32), 6: (64, 32), 7: (128, 32),
           9: (128, 64), 10: (64, 64), 11: (256, 128), 12: (128, 64), 13: (64, 32), 14: (128, 32), 15: (64, 64),
           16: (128, 64), 17: (64, 32), 18: (64, 128), 24: (256, 64), 25: (256, 64), 26: (128, 64), 56: (64, 128)}
KS = [(1, 1), (3, 1), (3, 2), (5, 1)]
GENERAL_MAP = (2, 13, 11)


@gpu
@pytest.mark.parametrize('k,s', KS)
@pytest.mark.parametrize('dtype', DT16)
@pytest.mark.parametrize('tile', sorted(GENERAL))
def test_exact_general_tiles(device, tile, dtype, k, s):
    """Every general 16-bit tile (register-staged 1-7, LDS-DMA 9-18, 24-26, 56): ragged pixel tail,
    image borders, input and output channel slices."""
    cout, cin = GENERAL[tile]
    o = operands(dtype, *GENERAL_MAP, cin, k, s)
    run_acts(device, o, tile, cout, f"tile {tile} dtype {dtype} k{k} s{s}")


def f32_operands(k, s):
    """Tile 8's operands: the bf16 cases' (cin 64), typed fp32."""
    ob = operands(L.DT_BF16, *GENERAL_MAP, 64, k, s)
    return types.SimpleNamespace(**{**vars(ob), 'dtype': L.DT_F32})


@gpu
@pytest.mark.parametrize('k,s', KS)
def test_exact_f32_tile8(device, k, s):
    """Tile 8 (fp32 FMA chain) on the bf16 cases' operands: the fp32 output is the exact sum."""
    o = f32_operands(k, s)
    for act, slope in ACTS:
        ref = apply_act(o.z[:, :64], act, slope)
        got = launch(device, o, 8, 64, act, slope)
        check_inputs(ref, torch.float32)
        assert_bits(got, expected(ref, torch.float32), f"tile 8 k{k} s{s} act {act} slope {slope}")


SPECIAL = [(19, 2, 16, 16, 64, 64, 3, 1), (19, 2, 32, 48, 64, 64, 3, 1), (20, 2, 16, 16, 128, 256, 3, 1),
           (20, 2, 32, 48, 64, 128, 3, 1), (21, 2, 16, 16, 64, 128, 3, 1), (21, 2, 32, 48, 64, 128, 3, 1),
           (23, 2, 16, 16, 64, 64, 3, 1), (23, 2, 32, 48, 64, 64, 3, 1), (48, 2, 40, 40, 64, 64, 3, 1),
           (49, 2, 40, 40, 64, 128, 3, 1), (50, 2, 32, 64, 64, 128, 3, 2), (50, 2, 31, 63, 64, 128, 3, 2),
           (22, 2, 13, 11, 64, 64, 1, 1), (22, 2, 13, 11, 256, 128, 1, 1), (22, 2, 13, 11, 256, 256, 1, 1),
           (22, 2, 96, 96, 64, 64, 1, 1)]


@gpu
@pytest.mark.parametrize('dtype', DT16)
@pytest.mark.parametrize('tile,n,h,w,cin,cout,k,s', SPECIAL)
def test_exact_special_kernels(device, tile, n, h, w, cin, cout, k, s, dtype):
    """Halo 19-21, weight-stationary 23, band halo 48 / 49, tile 50 and the weight-resident 1x1
    (22, one and several tiles per persistent block) at their smallest legal maps."""
    o = operands(dtype, n, h, w, cin, k, s, cout=cout)
    run_acts(device, o, tile, cout, f"tile {tile} {h}x{w} dtype {dtype}")


VARIANTS = [(t, v) for t in (3, 7, 16, 18, 56, 20, 48) for v in ('residual', 'up2', 'nchw_f32', 'cout_below_pad')
            if not (v == 'nchw_f32' and t in (20, 48))]  # the halo tiles store NHWC only
VARIANT_WIDTH = {3: 64, 7: 128, 16: 128, 18: 64, 56: 64, 20: 128, 48: 64}
VARIANT_ACT = (L.ACT_LEAKY, 0.125)


def variant_case(tile, dtype, variant):
    """(operands, cout, cout_pad or None, layout, lead, residual float64 NHWC or None, reference) of one case."""
    h, w = (16, 16) if tile == 20 else (40, 40) if tile == 48 else (13, 11)
    cin = 32 if tile == 7 else 64
    width = VARIANT_WIDTH[tile]
    o = operands(dtype, 2, h, w, cin, 3, 1)
    act, slope = VARIANT_ACT
    if variant == 'residual':
        r = dyadic((2, o.ho, o.wo, width), -4, 4, 1 / 16, torch.Generator().manual_seed(tile))
        return o, width, None, L.OUT_NHWC, OUT_LEAD, r, apply_act(o.z[:, :width], act, slope) + r.permute(0, 3, 1, 2)
    if variant == 'up2':
        return o, width, None, L.OUT_NHWC_UP2, UP2_LEAD, None, apply_act(o.z[:, :width], act, slope)
    if variant == 'nchw_f32':  # 127 / 255 channels, padded to the next tile width, at plane offset 1
        cout = 2 * width - 1
        return o, cout, 2 * width, L.OUT_NCHW_F32, OUT_LEAD, None, apply_act(o.z[:, :cout], act, slope)
    cout = width - 8
    return o, cout, width, L.OUT_NHWC, OUT_LEAD, None, apply_act(o.z[:, :cout], act, slope)


@gpu
@pytest.mark.parametrize('dtype', DT16)
@pytest.mark.parametrize('tile,variant', VARIANTS)
def test_exact_epilogue_variants(device, tile, dtype, variant):
    """The epilogue's other stores: a residual on the 1/16 grid (the fp32 add is exact, one rounding; the
    residual a NaN-framed slice), the x2 upsample store, the fp32 NCHW store (the exact sum, no rounding at
    all; 127 / 255 of 128 / 256 channels at plane offset 1) and cout < cout_pad, padding rows live."""
    o, cout, cpad, layout, lead, r, ref = variant_case(tile, dtype, variant)
    tdt, (act, slope) = TDT[dtype], VARIANT_ACT
    what = f"tile {tile} dtype {dtype} {variant}"
    if layout != L.OUT_NCHW_F32:
        check_inputs(ref, tdt, what)
    got = launch(device, o, tile, cout, act, slope, lead=lead, residual=r, layout=layout, cpad=cpad)
    assert_bits(got, expected(ref, tdt, layout, lead), what)


UP2_BELOW_PAD = (16, 120, 128)  # tile, cout, cout_pad


@gpu
@pytest.mark.parametrize('dtype', DT16)
def test_exact_up2_cout_below_pad(device, dtype):
    """The x2 store with cout < cout_pad (tile 16, 120 of 128): it writes four pixels per result, so a
    spilled padding channel would land four times."""
    tile, cout, cpad = UP2_BELOW_PAD
    o = operands(dtype, *GENERAL_MAP, 64, 3, 1)
    act, slope = VARIANT_ACT
    ref = apply_act(o.z[:, :cout], act, slope)
    check_inputs(ref, TDT[dtype])
    got = launch(device, o, tile, cout, act, slope, lead=UP2_LEAD, layout=L.OUT_NHWC_UP2, cpad=cpad)
    assert_bits(got, expected(ref, TDT[dtype], L.OUT_NHWC_UP2, UP2_LEAD), f"tile {tile} up2 cout {cout} < {cpad}")


BELOW_PAD = [(22, 13, 11, 128, 248, 256, 1, 1), (23, 16, 32, 64, 48, 64, 3, 1), (49, 40, 40, 64, 120, 128, 3, 1),
             (50, 31, 63, 64, 96, 128, 3, 2)]
BELOW_PAD_ACT = (L.ACT_LEAKY, 0.25)


@gpu
@pytest.mark.parametrize('dtype', DT16)
@pytest.mark.parametrize('tile,h,w,cin,cout,cpad,k,s', BELOW_PAD)
def test_exact_cout_below_pad(device, tile, h, w, cin, cout, cpad, k, s, dtype):
    """cout < cout_pad on the kernels with their own epilogues (padding channels are computed on live
    rows and not stored)."""
    o = operands(dtype, 2, h, w, cin, k, s)
    act, slope = BELOW_PAD_ACT
    ref = apply_act(o.z[:, :cout], act, slope)
    check_inputs(ref, TDT[dtype])
    got = launch(device, o, tile, cout, act, slope, cpad=cpad)
    assert_bits(got, expected(ref, TDT[dtype]), f"tile {tile} cout {cout} < {cpad}")


SPLITK_SHAPES = [(256, 3, 1), (512, 1, 1), (128, 3, 2), (256, 3, 2)]  # cin, k, s
SPLITK_TILES = [(16, 128), (18, 64), (56, 64)]
SPLITK_ACT = (L.ACT_LEAKY, 0.125)


def splitk_residual(o, cout):
    return dyadic((2, o.ho, o.wo, cout), -4, 4, 1 / 16, torch.Generator().manual_seed(5))


@gpu
@pytest.mark.parametrize('dtype', DT16)
@pytest.mark.parametrize('cin,k,s', SPLITK_SHAPES)
@pytest.mark.parametrize('tile,cout', SPLITK_TILES)
def test_exact_splitk(device, tile, cout, cin, k, s, dtype):
    """k_split 2, 3, 4: the reduce's store is RNE(true sum) and equals the unsplit launch bit for bit
    (cin 128 / stride 2 on tile 16: the chunk-major K order); then a residual through the reduce, read
    from a NaN-framed slice."""
    o = operands(dtype, *GENERAL_MAP, cin, k, s)
    tdt, (act, slope) = TDT[dtype], SPLITK_ACT
    ref = apply_act(o.z[:, :cout], act, slope)
    check_inputs(ref, tdt)
    exp = expected(ref, tdt)
    unsplit = launch(device, o, tile, cout, act, slope)
    assert_bits(unsplit, exp, f"tile {tile} unsplit")
    for ks in (2, 3, 4):
        got = launch(device, o, tile, cout, act, slope, k_split=ks)
        assert_bits(got, exp, f"tile {tile} k_split {ks}")
        assert torch.equal(got.view(torch.int16), unsplit.view(torch.int16))
    r = splitk_residual(o, cout)
    ref = ref + r.permute(0, 3, 1, 2)
    check_inputs(ref, tdt)
    assert_bits(launch(device, o, tile, cout, act, slope, k_split=3, residual=r), expected(ref, tdt),
                f"tile {tile} k_split 3 + residual")


KCM = [(2, 40, 40, 128), (1, 33, 47, 120)]  # n, h, w, cout


@gpu
@pytest.mark.parametrize('dtype', DT16)
@pytest.mark.parametrize('n,h,w,cout', KCM)
def test_exact_tile16_s2_cin128_chunk_major(device, n, h, w, cout, dtype):
    """Tile 16's chunk-major paired-tap K order (3x3 / s2 at cin 128), unsplit: odd map sizes put taps
    outside the image; several pixel tiles; cout < cout_pad."""
    o = operands(dtype, n, h, w, 128, 3, 2)
    run_acts(device, o, 16, cout, f"tile 16 KCM {h}x{w}")


POOL = [(16, 128, 64), (16, 128, 256), (18, 64, 64), (18, 64, 256), (25, 256, 64), (25, 256, 256)]  # tile, cout, cin


@gpu
@pytest.mark.parametrize('dtype', DT16)
@pytest.mark.parametrize('tile,cout,cin', POOL)
def test_exact_fused_pool(device, tile, cout, cin, dtype):
    """in_pool: the k2 s2 max-pool formed in the operand staging is exact on the grid, so the
    pooled 1x1 conv is RNE(true sum) like any other; the (2h, 2w) map is framed like any input."""
    o = operands(dtype, *GENERAL_MAP, cin, 1, 1, pool=True)
    run_acts(device, o, tile, cout, f"tile {tile} in_pool cin {cin}")


def _desc_1x1(n, h, w, cin, cout, cpad, in_off, in_stride, out_off, out_stride, act, slope, dtype):
    d = L.ConvDesc()
    d.n, d.h, d.w, d.cin, d.in_c_off, d.in_c_stride = n, h, w, cin, in_off, in_stride
    d.ho, d.wo, d.cout, d.cout_pad, d.out_c_off, d.out_c_stride = h, w, cout, cpad, out_off, out_stride
    d.kh = d.kw = 1
    d.stride, d.pad, d.act, d.leaky_slope, d.dtype, d.out_layout = 1, 0, act, slope, dtype, L.OUT_NHWC
    return d


PAIR = [(64, 128, True), (128, 120, False), (256, 256, True)]  # cin, cout2, y1 stored
PAIR_MAP = (2, 13, 11)
PAIR_ACT2 = (L.ACT_LEAKY, 0.25)


@functools.lru_cache(maxsize=None)
def pair_case(dtype, cin, cout2):
    """Operands, references and descriptors of one ycx_conv2d_pair case (CPU only; docstring of the test)."""
    n, h, w = PAIR_MAP
    tdt = TDT[dtype]
    xm = 2.0 if cin == 256 else 4.0
    c = types.SimpleNamespace(o=operands(dtype, n, h, w, cin, 1, 1, grid=(1 / 4, 1 / 4, xm, 2.0)), u1=1 / 16)
    c.z1 = c.o.z  # 256 channels
    y1 = rne(c.z1, tdt).double()
    assert 256 * float(y1.abs().max()) / c.u1 * 1 < SPAN
    g = torch.Generator().manual_seed(cin)
    w2 = dyadic((cout2, 256), -1, 1, 1.0, g)
    b2 = dyadic((cout2,), -B_MAX, B_MAX, B_STEP, g)
    c.cpad2 = 128 if cout2 <= 128 else 256
    if c.cpad2 > cout2:  # live padding rows, drawn after (and apart from) the case's own operands
        gp = torch.Generator().manual_seed(1000 + cin)
        w2 = torch.cat([w2, dyadic((c.cpad2 - cout2, 256), -1, 1, 1.0, gp)])
        b2 = torch.cat([b2, dyadic((c.cpad2 - cout2,), -B_MAX, B_MAX, B_STEP, gp)])
        assert bool(w2[cout2:].any(1).all())
    z2 = apply_act(torch.einsum('nchw,oc->nohw', y1, w2) + b2[None, :, None, None], *PAIR_ACT2)
    c.z2, c.z2_pad, c.w2, c.b2 = z2[:, :cout2], z2[:, cout2:], w2, b2
    ya_stride = OUT_LEAD + 256 + OUT_TAIL
    c.da = _desc_1x1(n, h, w, cin, 256, 256, c.o.in_extra, c.o.x_full.shape[3], OUT_LEAD, ya_stride, L.ACT_NONE, 0.0,
                     dtype)
    c.db = _desc_1x1(n, h, w, 256, cout2, c.cpad2, OUT_LEAD, ya_stride, OUT_LEAD, OUT_LEAD + cout2 + OUT_TAIL,
                     *PAIR_ACT2, dtype)
    return c


@gpu
@pytest.mark.parametrize('dtype', DT16)
@pytest.mark.parametrize('cin,cout2,store1', PAIR)
def test_exact_conv2d_pair(device, cin, cout2, store1, dtype):
    """ycx_conv2d_pair: y1 = RNE(sum1) (act none), then the second conv on those elements with
    w2 in {-1, 0, 1} and bias on the 1/16 grid: y1 (when stored) and y2 bit-exact to the reference
    chain, both in framed buffers; y1's buffer untouched when it is not stored. y1's elements are
    multiples of u1 = step_x * step_w, so the second conv's span is 256 * max|y1|/u1 * 1 < 2^20, asserted
    from the reference. That bound caps y1 at 2^12 u1: an eleven-bit fp16 element then needs rounding only
    in the top of its range, so the >= 10 % rounded condition is asserted on y2 in both types and on y1 in
    bf16; fp16 y1 rounding is covered by every single-conv case."""
    n, h, w = PAIR_MAP
    tdt = TDT[dtype]
    c = pair_case(dtype, cin, cout2)
    o = c.o
    if dtype == L.DT_BF16:
        check_inputs(c.z1, tdt, "pair y1")
    check_inputs(c.z2, tdt, "pair y2")
    w1p = o.wt[:, :, 0, 0].to(tdt)
    xd = guarded(o.x_full.to(tdt), input_guard(c.da, tdt.itemsize), device)
    w1d, b1d, w2d, b2d = [t.to(device) for t in (w1p, o.b.float(), c.w2.to(tdt), c.b2.float())]
    ya = guarded_out(out_frame(n, h, w, 256, tdt), device)
    yb = guarded_out(out_frame(n, h, w, cout2, tdt), device)
    L.check(L.lib.ycx_conv2d_pair(ctypes.byref(c.da), ctypes.byref(c.db), xd.data_ptr(), w1d.data_ptr(), b1d.data_ptr(),
                                  ya.data_ptr() if store1 else None, w2d.data_ptr(), b2d.data_ptr(), yb.data_ptr(),
                                  L.stream_handle(device)))
    torch.cuda.synchronize()
    assert_bits(fetch_out(yb, SENTINEL, what="pair y2"), expected(c.z2, tdt), "pair y2")
    got_a = fetch_out(ya, SENTINEL, what="pair y1")
    if store1:
        assert_bits(got_a, expected(c.z1, tdt), "pair y1")
    else:
        assert_bits(got_a, out_frame(n, h, w, 256, tdt), "pair y1 (not stored)")


STEM_GRID = dict(sx=1 / 64, sw=1 / 32)  # 27 * 256 * 64 < 2^20; eight significand bits hold both exactly
STEM_SHAPES = [(17, 19, 32), (18, 32, 32), (9, 64, 64)]  # wo % 16 == 0: the MFMA stem
STEM_DTYPES = [L.DT_BF16, L.DT_F16, L.DT_F32]


def image_guard(pad, w):
    """Guard floats of an fp32 NCHW image (16-byte aligned behind it; the stems ask for 8)."""
    return guard_elems(pad, w, 1, 4)


@functools.lru_cache(maxsize=None)
def stem_case(h, w, cout, s):
    """Image, weights, bias (float64) and the exact pre-activation of one ycx_stem_conv case (CPU only)."""
    n, cin, k = 2, 3, 3
    assert 27 * (X_MAX / STEM_GRID['sx']) * (W_MAX / STEM_GRID['sw']) < SPAN
    g = torch.Generator().manual_seed(h * w + s)
    c = types.SimpleNamespace(n=n, h=h, w=w, s=s, cout=cout)
    c.x = dyadic((n, cin, h, w), -X_MAX, X_MAX, STEM_GRID['sx'], g)
    c.wt = dyadic((cout, cin, k, k), -W_MAX, W_MAX, STEM_GRID['sw'], g)
    c.b = dyadic((cout,), -B_MAX, B_MAX, B_STEP, g)
    for t in (c.x, c.wt):
        assert torch.equal(t.to(torch.bfloat16).double(), t) and torch.equal(t.to(torch.float16).double(), t)
    c.z = F.conv2d(c.x, c.wt, c.b, s, 1)
    c.ho, c.wo = c.z.shape[2:]
    return c


def stem_desc(c, dtype, act, slope):
    d = L.ConvDesc()
    d.n, d.h, d.w, d.cin, d.in_c_off, d.in_c_stride = c.n, c.h, c.w, 3, 0, 3
    d.ho, d.wo, d.cout, d.cout_pad = c.ho, c.wo, c.cout, c.cout
    d.out_c_off, d.out_c_stride = STEM_LEAD, STEM_LEAD + c.cout + OUT_TAIL
    d.kh = d.kw = 3
    d.stride, d.pad, d.act, d.leaky_slope, d.dtype, d.out_layout = c.s, 1, act, slope, dtype, L.OUT_NHWC
    return d


@gpu
@pytest.mark.parametrize('dtype', STEM_DTYPES)
@pytest.mark.parametrize('s', [1, 2])
@pytest.mark.parametrize('h,w,cout', STEM_SHAPES)
def test_exact_stem(device, h, w, cout, s, dtype):
    """ycx_stem_conv, scalar and MFMA: the fp32 image (between NaN guards) and weights sit on a grid that
    the in-kernel conversion to the element type keeps unchanged; the output is RNE(true sum)."""
    c = stem_case(h, w, cout, s)
    tdt = TDT[dtype]
    xd = guarded(c.x.float(), image_guard(1, w), device)
    wd, bd = c.wt.permute(2, 3, 1, 0).contiguous().float().to(device), c.b.float().to(device)
    for act, slope in ACTS:
        ref = apply_act(c.z, act, slope)
        check_inputs(ref, tdt, "stem")
        d = stem_desc(c, dtype, act, slope)
        yd = guarded_out(out_frame(c.n, c.ho, c.wo, cout, tdt, STEM_LEAD), device)
        L.check(L.lib.ycx_stem_conv(ctypes.byref(d), xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), yd.data_ptr(),
                                    L.stream_handle(device)))
        torch.cuda.synchronize()
        what = f"stem {h}x{w} s{s} dtype {dtype} act {act} {slope}"
        assert_bits(fetch_out(yd, SENTINEL, what=what), expected(ref, tdt, lead=STEM_LEAD), what)


def stem2_descs(n, h, w, dtype, stem_s, act, slope, cout):
    """ycx_stem_conv2's two descriptors (no device)."""
    sh, sw = (h - 1) // stem_s + 1, (w - 1) // stem_s + 1
    ho, wo = (sh - 1) // 2 + 1, (sw - 1) // 2 + 1
    ds, dc = L.ConvDesc(), L.ConvDesc()
    ds.n, ds.h, ds.w, ds.cin, ds.in_c_off, ds.in_c_stride = n, h, w, 3, 0, 3
    ds.ho, ds.wo, ds.cout, ds.cout_pad, ds.out_c_off, ds.out_c_stride = sh, sw, 32, 32, 0, 32
    ds.kh = ds.kw = 3
    ds.stride, ds.pad, ds.act, ds.leaky_slope, ds.dtype, ds.out_layout = stem_s, 1, act, slope, dtype, L.OUT_NHWC
    dc.n, dc.h, dc.w, dc.cin, dc.in_c_off, dc.in_c_stride = n, sh, sw, 32, 0, 32
    dc.ho, dc.wo, dc.cout, dc.cout_pad = ho, wo, cout, 64
    dc.out_c_off, dc.out_c_stride = STEM_LEAD, STEM_LEAD + cout + OUT_TAIL
    dc.kh = dc.kw = 3
    dc.stride, dc.pad, dc.act, dc.leaky_slope, dc.dtype, dc.out_layout = 2, 1, act, slope, dtype, L.OUT_NHWC
    return ds, dc


def run_stem2(device, dtype, stem_s, act, slope, x, ws, bs, wc, bc, cout):
    """ycx_stem_conv2 on float64 operands (ws [32][3][3][3], wc [64][32][3][3]: rows cout .. 64 are the
    live padding rows; bc [64]); the raw output buffer."""
    n, _, h, w = x.shape
    tdt = TDT[dtype]
    ds, dc = stem2_descs(n, h, w, dtype, stem_s, act, slope, cout)
    assert wc.shape[0] == 64 and bc.shape[0] == 64 and bool(wc.flatten(1).any(1).all())
    wcp = wc.permute(0, 2, 3, 1).contiguous().to(tdt)
    assert torch.equal(wcp.double(), wc.permute(0, 2, 3, 1))
    xd = guarded(x.float(), image_guard(1, w), device)
    yd = guarded_out(out_frame(n, dc.ho, dc.wo, cout, tdt, STEM_LEAD), device)
    t = [v.to(device) for v in (ws.permute(2, 3, 1, 0).contiguous().float(), bs.float(), wcp, bc.float())]
    L.check(L.lib.ycx_stem_conv2(ctypes.byref(ds), ctypes.byref(dc), xd.data_ptr(), *[v.data_ptr() for v in t],
                                 yd.data_ptr(), L.stream_handle(device)))
    torch.cuda.synchronize()
    return fetch_out(yd, SENTINEL, what="stem2")


STEM2_ACTS = [(L.ACT_NONE, 0.0), (L.ACT_LEAKY, 0.125)]
STEM2 = [(1, 64, (2, 32, 64)), (2, 48, (2, 64, 128))]  # stem stride, cout, (n, h, w)


@functools.lru_cache(maxsize=None)
def stem2_case(dtype, stem_s, cout, nhw, act, slope):
    """Operands and references of one ycx_stem_conv2 case (CPU only; docstring of test_exact_stem2). wc and
    bc hold all 64 padded channels: rows cout .. 64 are drawn apart, on the same grid."""
    n, h, w = nhw
    tdt = TDT[dtype]
    g = torch.Generator().manual_seed(7 + stem_s)
    c = types.SimpleNamespace(cout=cout)
    if act == L.ACT_NONE:  # stem sums in units of 1/16
        c.x, c.ws, u = dyadic((n, 3, h, w), -4, 4, 1 / 4, g), dyadic((32, 3, 3, 3), -2, 2, 1 / 4, g), 1 / 16
        c.bs = dyadic((32,), -B_MAX, B_MAX, 1 / 16, g)
    else:                  # stem sums in units of 1/4, the stem map in units of slope / 4
        c.x, c.ws, u = dyadic((n, 3, h, w), -2, 2, 1 / 2, g), dyadic((32, 3, 3, 3), -1, 1, 1 / 2, g), slope / 4
        c.bs = dyadic((32,), -B_MAX, B_MAX, 1 / 4, g)
    wc = dyadic((cout, 32, 3, 3), -1, 1, 1 / 2, g)
    bc = dyadic((cout,), -B_MAX, B_MAX, B_STEP, g)
    if cout < 64:
        gp = torch.Generator().manual_seed(1007 + stem_s)
        wc = torch.cat([wc, dyadic((64 - cout, 32, 3, 3), -1, 1, 1 / 2, gp)])
        bc = torch.cat([bc, dyadic((64 - cout,), -B_MAX, B_MAX, B_STEP, gp)])
    c.wc, c.bc = wc, bc
    c.z1 = apply_act(F.conv2d(c.x, c.ws, c.bs, stem_s, 1), act, slope)
    mid = rne(c.z1, tdt).double()
    assert torch.equal(mid / u, (mid / u).round()) and 288 * float(mid.abs().max()) / u * 2 < SPAN
    z2 = apply_act(F.conv2d(mid, wc, bc, 2, 1), act, slope)
    c.ref, c.ref_pad = z2[:, :cout], z2[:, cout:]
    return c


@gpu
@pytest.mark.parametrize('dtype', DT16)
@pytest.mark.parametrize('act,slope', STEM2_ACTS)
@pytest.mark.parametrize('stem_s,cout,nhw', STEM2)
def test_exact_stem2(device, stem_s, cout, nhw, act, slope, dtype):
    """ycx_stem_conv2: the stem map is rounded to the element type as the kernel keeps it in LDS, the
    second conv (w2 in 1/2 steps within +-1) runs on those elements; output bit-exact. The second
    conv's span, 288 * max|mid|/u_mid * 2 < 2^20 with u_mid the stem's unit (x slope under leaky), is
    asserted from the reference. Act none: image and stem weights on the base grid, the bf16 stem map
    needs rounding (|mid| up to ~75 in units of 1/16). Leaky: the slope makes the unit 8 times finer,
    so image and stem weights move to 1/2 steps within +-2 / +-1 (no stem-map rounding there, nor in
    fp16, whose eleven bits hold every stem sum the span bound allows). cout 48: channels 48 .. 63 run on
    live rows."""
    tdt = TDT[dtype]
    c = stem2_case(dtype, stem_s, cout, nhw, act, slope)
    if act == L.ACT_NONE and dtype == L.DT_BF16:
        assert rounding_stats(c.z1, tdt)[0] >= MIN_ROUNDED  # the stem map's rounding is part of the case
    check_inputs(c.ref, tdt, "stem2")
    got = run_stem2(device, dtype, stem_s, act, slope, c.x, c.ws, c.bs, c.wc, c.bc, cout)
    assert_bits(got, expected(c.ref, tdt, lead=STEM_LEAD), f"stem2 s{stem_s} cout {cout} act {act} dtype {dtype}")


HEAD = [(2, 7, 7, 128), (3, 10, 8, 256), (2, 7, 7, 512), (2, 10, 8, 128)]  # n, h, w, cin
HEAD_NA, HEAD_NC = 3, 80
HEAD_COUT = HEAD_NA * (HEAD_NC + 5)
ROWS_SENTINEL = -7


def head_descs(o):
    d = _desc_1x1(o.n, o.h, o.w, o.cin, HEAD_COUT, 256, o.in_extra, o.x_full.shape[3], 0, HEAD_COUT, L.ACT_NONE, 0.0,
                  o.dtype)
    d.out_layout = L.OUT_NCHW_F32
    hd = L.HeadDesc()
    rows = HEAD_NA * o.h * o.w
    hd.na, hd.no, hd.nc, hd.rows_total, hd.row_off, hd.conf_thres = HEAD_NA, HEAD_NC + 5, HEAD_NC, rows, 0, 2.0
    for i in range(2 * HEAD_NA):
        hd.anchors_scaled[i] = 1.0 + i
    return d, hd


@gpu
@pytest.mark.parametrize('dtype', DT16)
@pytest.mark.parametrize('n,h,w,cin', HEAD)
def test_exact_head_raw_store(device, n, h, w, cin, dtype):
    """ycx_conv2d_head's raw-head store: cout 255 padded to 256 (row 255 live), 64-pixel tiles straddling
    image boundaries; conf_thres above 1 appends nothing, and the fp32 NCHW heads are the exact sums. The
    heads buffer has no stride of its own: it, cand and cand_rows start as sentinels, heads lies between
    sentinel guards, and nothing but heads may change."""
    o = operands(dtype, n, h, w, cin, 1, 1)
    tdt = TDT[dtype]
    ref = o.z[:, :HEAD_COUT]
    check_inputs(ref, torch.float32)
    assert not bool((ref == SENTINEL_F32).any())
    wp, bp = packed(o, HEAD_COUT, 256)
    d, hd = head_descs(o)
    rows = hd.rows_total
    xd = guarded(o.x_full.to(tdt), input_guard(d, tdt.itemsize), device)
    wd, bd = wp.reshape(256, cin).to(device), bp.to(device)
    heads = guarded_out(torch.full((n, HEAD_COUT, h, w), SENTINEL_F32), device)
    cand = torch.full((n, rows, 8), SENTINEL_F32, device=device)
    cand_rows = torch.full((n, rows), ROWS_SENTINEL, dtype=torch.int32, device=device)
    counts = torch.zeros(n, dtype=torch.int32, device=device)  # zeroed: the header's contract
    status = torch.zeros(1, dtype=torch.int32, device=device)
    L.check(L.lib.ycx_conv2d_head(ctypes.byref(d), ctypes.byref(hd), xd.data_ptr(), wd.data_ptr(), bd.data_ptr(),
                                  heads.data_ptr(), cand.data_ptr(), cand_rows.data_ptr(), counts.data_ptr(),
                                  status.data_ptr(), L.stream_handle(device)))
    torch.cuda.synchronize()
    assert not counts.any() and int(status) == 0
    assert bool((cand == SENTINEL_F32).all()) and bool((cand_rows == ROWS_SENTINEL).all())
    what = f"head cin {cin} {h}x{w} dtype {dtype}"
    assert_bits(fetch_out(heads, SENTINEL_F32, what=what), ref.float(), what)


# ---- SiLU and pre-scaled SiLU at ulp level ----
# z (the accumulator plus bias) is exact as above. The FAST epilogue (ycx_internal.h, ycx_act / act_t)
# rounds one multiply of the argument (SiLU: z * -log2(e), relative 2^-24, which moves 2^t by
# |t| ln2 2^-24 <= |z| 2^-24) and then evaluates hardware exp2 and rcp at 1 ulp (2^-23) each, one add
# or fma (2^-24) and the final multiply (2^-24): within (|z| + 4) 2^-23 relative of the true value.
# An element is held bit-exact where the float64 reference lies farther than twice that from a
# rounding boundary, and within one element-ulp of RNE(reference) everywhere.
LOG2E = 1.4426950408889634
SILU_MAX_Z = 32.0
MAX_EXCUSED = {torch.bfloat16: 0.01, torch.float16: 0.05}  # boundary spacing puts them at ~0.4 % / 2-3 %


def silu_ref(z, act):
    if act == L.ACT_SILU_PS:  # z = -log2(e) c: c / (1 + 2^z)
        return (-z / LOG2E) / (1 + torch.exp2(z))
    return z / (1 + torch.exp(-z))


def silu_conditions(z, act, tdt, what=""):
    """From the exact NCHW pre-activation alone: the NHWC float64 reference, the elements excused by
    the margin and the fp16 subnormal results; asserts the input conditions."""
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


def check_silu(got, z, act, tdt, what, lead=OUT_LEAD, tail=OUT_TAIL):
    """got: the raw framed NHWC output buffer (the slice at channel ``lead``, ``tail`` channels behind it,
    the sentinel in both, bit for bit); z: the exact pre-activation NCHW (of the packed operands).
    Elements of the slice are compared as values: +0 and -0 (silu(0) of either sign) coincide."""
    ref, excused, sub, share = silu_conditions(z, act, tdt, what)
    c = ref.shape[3]
    assert got.shape == (*ref.shape[:3], lead + c + tail) and got.dtype == tdt
    frame = got.clone()
    frame[..., lead:lead + c] = SENTINEL
    assert_bits(frame, torch.full_like(got, SENTINEL), f"{what}: wrote outside the output channel slice")
    g = got[..., lead:lead + c].contiguous()
    ulps = elt_ulps(g, rne(ref, tdt), tdt)
    if sub.any():  # fp16 subnormal results: an absolute bound, counted apart
        assert float((g.double() - ref).abs()[sub].max()) <= 2.0 ** -24, what
    assert int(ulps[~sub].abs().max()) <= 1, f"{what}: {int(ulps[~sub].abs().max())} element-ulps from RNE(ref)"
    must = ~excused & ~sub
    bad = must & (ulps != 0)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {int(must.sum())} elements away from a rounding " \
                          f"boundary differ from RNE(ref) ({share:.4f} excused, {int(sub.sum())} subnormal)"


def silu_operands(dtype, n, h, w, cin, k, s, cout):
    """x in steps of 1/8 of its half-range hx = 2^floor(log2(12 / sqrt(K))) (z of a few units), w in 1/8 steps
    within +-1, bias in 1/16 steps within +-1: K * 8 * 8 < 2^20."""
    K = cin * k * k
    hx = 2.0 ** math.floor(math.log2(12 / math.sqrt(K)))
    return operands(dtype, n, h, w, cin, k, s, grid=(hx / 8, 1 / 8, hx, 1.0), cout=cout, seed=3)


SILU_ACTS = [L.ACT_SILU, L.ACT_SILU_PS]
SILU_CASES = [(3, 2, 13, 11, 64, 64, 3, 1, 0), (16, 2, 13, 11, 64, 128, 3, 1, 0), (18, 2, 13, 11, 64, 64, 3, 1, 0),
              (20, 2, 16, 16, 64, 128, 3, 1, 0), (22, 2, 13, 11, 64, 64, 1, 1, 0), (23, 2, 16, 16, 64, 64, 3, 1, 0),
              (50, 2, 32, 64, 64, 128, 3, 2, 0), (16, 2, 13, 11, 256, 128, 1, 1, 2)]  # last: the split-K reduce


@gpu
@pytest.mark.parametrize('act', SILU_ACTS)
@pytest.mark.parametrize('dtype', DT16)
@pytest.mark.parametrize('tile,n,h,w,cin,cout,k,s,k_split', SILU_CASES)
def test_silu_ulps(device, tile, n, h, w, cin, cout, k, s, k_split, dtype, act):
    """One tile of each epilogue family: register-staged 3, LDS-DMA 16 / 18, halo 20, weight-resident
    22, 23, 50 and the split-K reduce. YCX_ACT_SILU_PS: the packed weights and bias themselves are on
    the grid (z is the packed conv's sum)."""
    o = silu_operands(dtype, n, h, w, cin, k, s, cout)
    got = launch(device, o, tile, cout, act, 0.0, k_split=k_split)
    check_silu(got, o.z[:, :cout], act, TDT[dtype], f"tile {tile} dtype {dtype} act {act}")


def stem2_silu_operands(act, dtype):
    """A stem whose SiLU output is determined whatever the epilogue's last bits: image in {0, 1},
    stem weights in {0, +-1/4} and one bias b0 give a few dozen distinct pre-activations b0 <= |z1| <=
    b0 + 6.75 in 1/4 steps, every SiLU value in [8, 16). b0 is the first of 9 (pre-scaled: 12), + 1/16,
    ... for which -- from the reference alone -- every value lies farther than the margin from a rounding
    boundary, so the stem map is RNE(silu(z1)) exactly. The second conv (w2 in 1/64 steps within
    +-1/64) then has an exact z2 with 288 * max|mid|/u_mid * 1 < 2^20."""
    tdt = TDT[dtype]
    sgn, b0 = (-1.0, 12.0) if act == L.ACT_SILU_PS else (1.0, 9.0)
    g = torch.Generator().manual_seed(11)
    x = dyadic((2, 3, 32, 64), 0, 1, 1.0, g)
    ws = sgn * dyadic((32, 3, 3, 3), 0, 1 / 4, 1 / 4, g)
    s0 = F.conv2d(x, ws, None, 1, 1)
    for i in range(16):
        bs = torch.full((32,), sgn * (b0 + i / 16), dtype=torch.float64)
        z1 = s0 + bs[None, :, None, None]
        ref1 = silu_ref(z1, act)
        lo, hi = elt_neighbours(ref1, tdt)
        margin = (z1.abs() + 8) * 2.0 ** -23 * ref1.abs()
        if bool(((lo == hi) | ((ref1 - (lo + hi) / 2).abs() > margin)).all()):
            break
    else:
        raise AssertionError("no bias keeps every stem value off the rounding boundaries")
    mid = rne(ref1, tdt).double()
    u = 2.0 ** -4 if tdt == torch.bfloat16 else 2.0 ** -7  # element spacing in [8, 16)
    assert float(mid.min()) >= 8 and float(mid.max()) < 16 and 288 * 16 / u * 1 < SPAN
    wc = dyadic((64, 32, 3, 3), -1 / 64, 1 / 64, 1 / 64, g)
    bc = dyadic((64,), -1, 1, B_STEP, g)
    z2 = F.conv2d(mid, wc, bc, 2, 1)
    return x, ws, bs, wc, bc, z2


@gpu
@pytest.mark.parametrize('act', SILU_ACTS)
@pytest.mark.parametrize('dtype', DT16)
def test_silu_ulps_stem2(device, dtype, act):
    """stem2's two SiLU epilogues: the stem map must be RNE(silu) (any other element moves z2 by far
    more than an ulp), the output is held to the ulp bar."""
    x, ws, bs, wc, bc, z2 = stem2_silu_operands(act, dtype)
    got = run_stem2(device, dtype, 1, act, 0.0, x, ws, bs, wc, bc, 64)
    check_silu(got, z2, act, TDT[dtype], f"stem2 dtype {dtype} act {act}", lead=STEM_LEAD)
