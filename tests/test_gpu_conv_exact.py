"""Bit-exact conv parity on exactly representable operands ("exact-operand bar").

Operands and bias are small dyadic rationals, so every product and every partial sum is exactly
representable in fp32: the accumulator holds the true sum whatever the tile's K order, split-K
split or MFMA grouping, and the stored element must be RNE(true sum) bit for bit -- no tolerance.
The reference is torch's float64 conv on the CPU; the element reference is its cast (helpers.rne).

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
  1-7, 9-18, 24-26, 56   test_exact_general_tiles: n 2, 13 x 11, in_extra 8, out_extra 16,
                         (k, s) in (1,1) (3,1) (3,2) (5,1); act none, leaky 0.125, leaky 0.25
  8                      test_exact_f32_tile8 (the same operands)
  19, 20, 21, 23         test_exact_special_kernels 16 x 16 and 32 x 48
  48, 49                 test_exact_special_kernels 40 x 40
  50                     test_exact_special_kernels 32 x 64 and 31 x 63
  22                     test_exact_special_kernels 13 x 11 (cin 64 / 256) and n 2, 96 x 96
  3, 7, 16, 18, 56, 20, 48   test_exact_epilogue_variants (residual, x2 upsample, fp32 NCHW, cout < cout_pad)
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

from helpers import dyadic, elt_neighbours, elt_ulps, rne, rounding_stats

pytestmark = pytest.mark.gpu

L = pytest.importorskip("ycx._lib")

TDT = {L.DT_BF16: torch.bfloat16, L.DT_F16: torch.float16, L.DT_F32: torch.float32}
DT16 = [L.DT_BF16, L.DT_F16]
SPAN = 1 << 20                    # K * max|x|/step_x * max|w|/step_w stays below this
MIN_ROUNDED, MIN_TIES = 0.10, 0.01
ACTS = [(L.ACT_NONE, 0.0), (L.ACT_LEAKY, 0.125), (L.ACT_LEAKY, 0.25)]  # both slopes exact, neither is 0.1
X_MAX, W_MAX, B_MAX, B_STEP = 4.0, 2.0, 2.0, 1 / 16
_FP16_GRIDS = [(1 / 16, 1 / 8), (1 / 8, 1 / 8), (1 / 8, 1 / 4), (1 / 4, 1 / 4)]


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


def assert_bits(got, exp, what=""):
    """torch.equal on the bit patterns; on a mismatch, say how many elements and how far."""
    it = torch.int32 if got.dtype == torch.float32 else torch.int16
    assert got.shape == exp.shape and got.dtype == exp.dtype
    if torch.equal(got.contiguous().view(it), exp.contiguous().view(it)):
        return
    bad = got.contiguous().view(it) != exp.contiguous().view(it)
    d = elt_ulps(got, exp, got.dtype)[bad]
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from RNE(true sum); "
                         f"distance in representable values: min {int(d.min())}, max {int(d.max())}; "
                         f"first at {[int(v) for v in bad.nonzero()[0]]}")


@functools.lru_cache(maxsize=None)
def operands(dtype, n, h, w, cin, k, s, in_extra=8, pool=False, seed=0, grid=None, cout=256):
    """Operands of one conv (shared by every tile / act / variant that runs it; never modified):
    x_full [n][h][w][in_extra + cin] NHWC float64, wt [cout][cin][k][k], b [cout] and the exact
    pre-activation z [n][cout][ho][wo]. pool: x_full is the (2h, 2w) map of the fused max-pool.
    grid: (step_x, step_w, max|x|, max|w|) where a case needs another than pick_grid's."""
    sx, sw, xm, wm = grid or (pick_grid(cin * k * k, dtype) + (X_MAX, W_MAX))
    assert cin * k * k * (xm / sx) * (wm / sw) < SPAN
    g = torch.Generator().manual_seed(1000 * seed + 17 * cin + k + s)
    up = 2 if pool else 1
    o = types.SimpleNamespace(n=n, h=h, w=w, cin=cin, k=k, s=s, in_extra=in_extra, pool=pool, dtype=dtype)
    o.x_full = dyadic((n, up * h, up * w, in_extra + cin), -xm, xm, sx, g)
    o.wt = dyadic((cout, cin, k, k), -wm, wm, sw, g)
    o.b = dyadic((cout,), -B_MAX, B_MAX, B_STEP, g)
    tdt = TDT[dtype]
    for t in (o.x_full, o.wt):  # the element type holds the operands exactly
        assert torch.equal(t.to(tdt).double(), t)
    x = o.x_full[..., in_extra:].permute(0, 3, 1, 2)
    if pool:
        x = F.max_pool2d(x, 2, 2)  # exact
    o.z = F.conv2d(x, o.wt, o.b, s, k // 2)
    o.ho, o.wo = o.z.shape[2:]
    return o


def cpad_of(cout, dtype):
    if dtype == L.DT_F32:
        return -(-cout // 64) * 64
    return 32 if cout <= 32 else 64 if cout <= 64 else -(-cout // 128) * 128


def launch(device, o, tile, cout, act=L.ACT_NONE, slope=0.0, out_extra=16, residual=None, layout=L.OUT_NHWC,
           k_split=0, cpad=None):
    """One conv through the C ABI on operands ``o`` (first ``cout`` channels); the raw output buffer."""
    tdt = TDT[o.dtype]
    cpad = cpad or cpad_of(cout, o.dtype)
    wp = torch.zeros(cpad, o.k, o.k, o.cin, dtype=tdt)
    wp[:cout] = o.wt[:cout].permute(0, 2, 3, 1).to(tdt)
    bp = torch.zeros(cpad)
    bp[:cout] = o.b[:cout].float()
    up = 2 if layout == L.OUT_NHWC_UP2 else 1
    if layout == L.OUT_NCHW_F32:
        y = torch.zeros(o.n, cout, o.ho, o.wo, dtype=torch.float32)
    else:
        y = torch.zeros(o.n, o.ho * up, o.wo * up, cout + out_extra, dtype=tdt)
    d = L.ConvDesc()
    d.n, d.h, d.w, d.cin, d.in_c_off, d.in_c_stride = o.n, o.h, o.w, o.cin, o.in_extra, o.cin + o.in_extra
    d.ho, d.wo, d.cout, d.cout_pad = o.ho, o.wo, cout, cpad
    d.out_c_off, d.out_c_stride = (0, cout) if layout == L.OUT_NCHW_F32 else (out_extra, cout + out_extra)
    d.kh = d.kw = o.k
    d.stride, d.pad, d.act, d.leaky_slope = o.s, 0 if o.pool else o.k // 2, act, slope
    d.dtype, d.out_layout, d.tile, d.k_split, d.in_pool = o.dtype, layout, tile, k_split, int(o.pool)
    d.res_c_off, d.res_c_stride = 0, cout
    xd, wd, bd, yd = o.x_full.to(tdt).to(device), wp.to(device), bp.to(device), y.to(device)
    rd = residual.to(tdt).to(device) if residual is not None else None
    st = L.stream_handle(device)
    if k_split > 1:
        nws = int(L.lib.ycx_conv_workspace_size(ctypes.byref(d)))
        assert nws == k_split * o.n * o.ho * o.wo * cpad * 4
        ws = torch.full((nws // 4,), float('nan'), device=device)  # every partial must be overwritten
        L.check(L.lib.ycx_conv2d_ws(ctypes.byref(d), xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), yd.data_ptr(),
                                    L.ptr(rd), ws.data_ptr(), nws, st))
    else:
        L.check(L.lib.ycx_conv2d(ctypes.byref(d), xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), yd.data_ptr(),
                                 L.ptr(rd), st))
    torch.cuda.synchronize()
    return yd.cpu()


def expected(ref64, tdt, layout=L.OUT_NHWC, out_extra=16):
    """The whole output buffer: RNE(ref) in the channel slice, zeros outside it."""
    if layout == L.OUT_NCHW_F32:
        check_inputs(ref64, torch.float32)
        return ref64.float()
    r = ref64.permute(0, 2, 3, 1)
    if layout == L.OUT_NHWC_UP2:
        r = r.repeat_interleave(2, 1).repeat_interleave(2, 2)
    exp = torch.zeros(*r.shape[:3], r.shape[3] + out_extra, dtype=tdt)
    exp[..., out_extra:] = rne(r, tdt)
    return exp


def run_acts(device, o, tile, cout, what, **kw):
    """act none, leaky 0.125 and leaky 0.25 of one conv, each bit-exact."""
    tdt = TDT[o.dtype]
    for act, slope in ACTS:
        ref = apply_act(o.z[:, :cout], act, slope)
        check_inputs(ref, tdt, what)
        got = launch(device, o, tile, cout, act, slope, **kw)
        assert_bits(got, expected(ref, tdt, out_extra=kw.get('out_extra', 16)), f"{what} act {act} slope {slope}")


# tile -> (cout, cin) of the general cases (cout = the tile's channel width, cin its K step or twice it)
GENERAL = {1: (128, 64), 2: (64, 64), 3: (64, 64), 4: (128, 64), 5: (32, 32), 6: (64, 32), 7: (128, 32),
           9: (128, 64), 10: (64, 64), 11: (256, 128), 12: (128, 64), 13: (64, 32), 14: (128, 32), 15: (64, 64),
           16: (128, 64), 17: (64, 32), 18: (64, 128), 24: (256, 64), 25: (256, 64), 26: (128, 64), 56: (64, 128)}
KS = [(1, 1), (3, 1), (3, 2), (5, 1)]


@pytest.mark.parametrize('k,s', KS)
@pytest.mark.parametrize('dtype', DT16)
@pytest.mark.parametrize('tile', sorted(GENERAL))
def test_exact_general_tiles(device, tile, dtype, k, s):
    """Every general 16-bit tile (register-staged 1-7, LDS-DMA 9-18, 24-26, 56): ragged pixel tail,
    image borders, input and output channel slices."""
    cout, cin = GENERAL[tile]
    o = operands(dtype, 2, 13, 11, cin, k, s)
    run_acts(device, o, tile, cout, f"tile {tile} dtype {dtype} k{k} s{s}")


@pytest.mark.parametrize('k,s', KS)
def test_exact_f32_tile8(device, k, s):
    """Tile 8 (fp32 FMA chain) on the bf16 cases' operands: the fp32 output is the exact sum."""
    ob = operands(L.DT_BF16, 2, 13, 11, 64, k, s)
    o = types.SimpleNamespace(**{**vars(ob), 'dtype': L.DT_F32})
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


@pytest.mark.parametrize('dtype', DT16)
@pytest.mark.parametrize('tile,n,h,w,cin,cout,k,s', SPECIAL)
def test_exact_special_kernels(device, tile, n, h, w, cin, cout, k, s, dtype):
    """Halo 19-21, weight-stationary 23, band halo 48 / 49, tile 50 and the weight-resident 1x1
    (22, one and several tiles per persistent block) at their smallest legal maps."""
    o = operands(dtype, n, h, w, cin, k, s, cout=cout)
    run_acts(device, o, tile, cout, f"tile {tile} {h}x{w} dtype {dtype}")


VARIANTS = [(t, v) for t in (3, 7, 16, 18, 56, 20, 48) for v in ('residual', 'up2', 'nchw_f32', 'cout_below_pad')
            if not (v == 'nchw_f32' and t in (20, 48))]  # the halo tiles store NHWC only


@pytest.mark.parametrize('dtype', DT16)
@pytest.mark.parametrize('tile,variant', VARIANTS)
def test_exact_epilogue_variants(device, tile, dtype, variant):
    """The epilogue's other stores: a residual on the 1/16 grid (the fp32 add is exact, one rounding),
    the x2 upsample store, the fp32 NCHW store (the exact sum, no rounding at all) and cout < cout_pad."""
    h, w = (16, 16) if tile == 20 else (40, 40) if tile == 48 else (13, 11)
    cin = 32 if tile == 7 else 64
    width = {3: 64, 7: 128, 16: 128, 18: 64, 56: 64, 20: 128, 48: 64}[tile]
    o = operands(dtype, 2, h, w, cin, 3, 1)
    tdt, act, slope = TDT[dtype], L.ACT_LEAKY, 0.125
    what = f"tile {tile} dtype {dtype} {variant}"
    if variant == 'residual':
        r = dyadic((2, o.ho, o.wo, width), -4, 4, 1 / 16, torch.Generator().manual_seed(tile))
        ref = apply_act(o.z[:, :width], act, slope) + r.permute(0, 3, 1, 2)
        check_inputs(ref, tdt, what)
        got = launch(device, o, tile, width, act, slope, residual=r)
        assert_bits(got, expected(ref, tdt), what)
    elif variant == 'up2':
        ref = apply_act(o.z[:, :width], act, slope)
        check_inputs(ref, tdt, what)
        got = launch(device, o, tile, width, act, slope, layout=L.OUT_NHWC_UP2, out_extra=8)
        assert_bits(got, expected(ref, tdt, L.OUT_NHWC_UP2, 8), what)
    elif variant == 'nchw_f32':
        cout = 2 * width - 1  # 127 / 255 channels, padded to the next tile width
        ref = apply_act(o.z[:, :cout], act, slope)
        got = launch(device, o, tile, cout, act, slope, layout=L.OUT_NCHW_F32, cpad=2 * width)
        assert_bits(got, expected(ref, tdt, L.OUT_NCHW_F32), what)
    else:
        cout = width - 8
        ref = apply_act(o.z[:, :cout], act, slope)
        check_inputs(ref, tdt, what)
        got = launch(device, o, tile, cout, act, slope, cpad=width)
        assert_bits(got, expected(ref, tdt), what)


@pytest.mark.parametrize('dtype', DT16)
@pytest.mark.parametrize('tile,h,w,cin,cout,cpad,k,s', [(22, 13, 11, 128, 248, 256, 1, 1), (23, 16, 32, 64, 48, 64, 3, 1),
                                                        (49, 40, 40, 64, 120, 128, 3, 1), (50, 31, 63, 64, 96, 128, 3, 2)])
def test_exact_cout_below_pad(device, tile, h, w, cin, cout, cpad, k, s, dtype):
    """cout < cout_pad on the kernels with their own epilogues (padding channels are not stored)."""
    o = operands(dtype, 2, h, w, cin, k, s)
    ref = apply_act(o.z[:, :cout], L.ACT_LEAKY, 0.25)
    check_inputs(ref, TDT[dtype])
    got = launch(device, o, tile, cout, L.ACT_LEAKY, 0.25, cpad=cpad)
    assert_bits(got, expected(ref, TDT[dtype]), f"tile {tile} cout {cout} < {cpad}")


@pytest.mark.parametrize('dtype', DT16)
@pytest.mark.parametrize('cin,k,s', [(256, 3, 1), (512, 1, 1), (128, 3, 2), (256, 3, 2)])
@pytest.mark.parametrize('tile,cout', [(16, 128), (18, 64), (56, 64)])
def test_exact_splitk(device, tile, cout, cin, k, s, dtype):
    """k_split 2, 3, 4: the reduce's store is RNE(true sum) and equals the unsplit launch bit for bit
    (cin 128 / stride 2 on tile 16: the chunk-major K order); then a residual through the reduce."""
    o = operands(dtype, 2, 13, 11, cin, k, s)
    tdt, act, slope = TDT[dtype], L.ACT_LEAKY, 0.125
    ref = apply_act(o.z[:, :cout], act, slope)
    check_inputs(ref, tdt)
    exp = expected(ref, tdt)
    unsplit = launch(device, o, tile, cout, act, slope)
    assert_bits(unsplit, exp, f"tile {tile} unsplit")
    for ks in (2, 3, 4):
        got = launch(device, o, tile, cout, act, slope, k_split=ks)
        assert_bits(got, exp, f"tile {tile} k_split {ks}")
        assert torch.equal(got.view(torch.int16), unsplit.view(torch.int16))
    r = dyadic((2, o.ho, o.wo, cout), -4, 4, 1 / 16, torch.Generator().manual_seed(5))
    ref = ref + r.permute(0, 3, 1, 2)
    check_inputs(ref, tdt)
    assert_bits(launch(device, o, tile, cout, act, slope, k_split=3, residual=r), expected(ref, tdt),
                f"tile {tile} k_split 3 + residual")


@pytest.mark.parametrize('dtype', DT16)
@pytest.mark.parametrize('n,h,w,cout', [(2, 40, 40, 128), (1, 33, 47, 120)])
def test_exact_tile16_s2_cin128_chunk_major(device, n, h, w, cout, dtype):
    """Tile 16's chunk-major paired-tap K order (3x3 / s2 at cin 128), unsplit: odd map sizes put taps
    outside the image; several pixel tiles; cout < cout_pad."""
    o = operands(dtype, n, h, w, 128, 3, 2)
    run_acts(device, o, 16, cout, f"tile 16 KCM {h}x{w}")


@pytest.mark.parametrize('dtype', DT16)
@pytest.mark.parametrize('tile,cout,cin', [(16, 128, 64), (16, 128, 256), (18, 64, 64), (18, 64, 256), (25, 256, 64),
                                           (25, 256, 256)])
def test_exact_fused_pool(device, tile, cout, cin, dtype):
    """in_pool: the k2 s2 max-pool formed in the operand staging is exact on the grid, so the
    pooled 1x1 conv is RNE(true sum) like any other."""
    o = operands(dtype, 2, 13, 11, cin, 1, 1, pool=True)
    run_acts(device, o, tile, cout, f"tile {tile} in_pool cin {cin}")


def _desc_1x1(n, h, w, cin, cout, cpad, in_off, in_stride, out_off, out_stride, act, slope, dtype):
    d = L.ConvDesc()
    d.n, d.h, d.w, d.cin, d.in_c_off, d.in_c_stride = n, h, w, cin, in_off, in_stride
    d.ho, d.wo, d.cout, d.cout_pad, d.out_c_off, d.out_c_stride = h, w, cout, cpad, out_off, out_stride
    d.kh = d.kw = 1
    d.stride, d.pad, d.act, d.leaky_slope, d.dtype, d.out_layout = 1, 0, act, slope, dtype, L.OUT_NHWC
    return d


@pytest.mark.parametrize('dtype', DT16)
@pytest.mark.parametrize('cin,cout2,store1', [(64, 128, True), (128, 120, False), (256, 256, True)])
def test_exact_conv2d_pair(device, cin, cout2, store1, dtype):
    """ycx_conv2d_pair: y1 = RNE(sum1) (act none), then the second conv on those elements with
    w2 in {-1, 0, 1} and bias on the 1/16 grid: y1 (when stored) and y2 bit-exact to the reference
    chain. y1's elements are multiples of u1 = step_x * step_w, so the second conv's span is
    256 * max|y1|/u1 * 1 < 2^20, asserted from the reference. That bound caps y1 at 2^12 u1: an
    eleven-bit fp16 element then needs rounding only in the top of its range, so the >= 10 % rounded
    condition is asserted on y2 in both types and on y1 in bf16; fp16 y1 rounding is covered by every
    single-conv case."""
    n, h, w = 2, 13, 11
    tdt = TDT[dtype]
    xm = 2.0 if cin == 256 else 4.0
    o = operands(dtype, n, h, w, cin, 1, 1, grid=(1 / 4, 1 / 4, xm, 2.0))
    u1 = 1 / 16
    z1 = o.z  # 256 channels
    if dtype == L.DT_BF16:
        check_inputs(z1, tdt, "pair y1")
    y1 = rne(z1, tdt).double()
    assert 256 * float(y1.abs().max()) / u1 * 1 < SPAN
    g = torch.Generator().manual_seed(cin)
    w2 = dyadic((cout2, 256), -1, 1, 1.0, g)
    b2 = dyadic((cout2,), -B_MAX, B_MAX, B_STEP, g)
    z2 = apply_act(torch.einsum('nchw,oc->nohw', y1, w2) + b2[None, :, None, None], L.ACT_LEAKY, 0.25)
    check_inputs(z2, tdt, "pair y2")
    cpad2 = 128 if cout2 <= 128 else 256
    w1p = o.wt[:, :, 0, 0].to(tdt)
    w2p = torch.zeros(cpad2, 256, dtype=tdt)
    w2p[:cout2] = w2.to(tdt)
    b2p = torch.zeros(cpad2)
    b2p[:cout2] = b2.float()
    xd, w1d, b1d, w2d, b2d = [t.to(device) for t in (o.x_full.to(tdt), w1p, o.b.float(), w2p, b2p)]
    ya = torch.zeros(n, h, w, 256 + 16, dtype=tdt, device=device)
    yb = torch.zeros(n, h, w, cout2 + 8, dtype=tdt, device=device)
    da = _desc_1x1(n, h, w, cin, 256, 256, 8, cin + 8, 16, 272, L.ACT_NONE, 0.0, dtype)
    db = _desc_1x1(n, h, w, 256, cout2, cpad2, 16, 272, 8, cout2 + 8, L.ACT_LEAKY, 0.25, dtype)
    L.check(L.lib.ycx_conv2d_pair(ctypes.byref(da), ctypes.byref(db), xd.data_ptr(), w1d.data_ptr(), b1d.data_ptr(),
                                  ya.data_ptr() if store1 else None, w2d.data_ptr(), b2d.data_ptr(), yb.data_ptr(),
                                  L.stream_handle(device)))
    torch.cuda.synchronize()
    assert_bits(yb.cpu(), expected(z2, tdt, out_extra=8), "pair y2")
    if store1:
        assert_bits(ya.cpu(), expected(z1, tdt, out_extra=16), "pair y1")
    else:
        assert not ya.any()


STEM_GRID = dict(sx=1 / 64, sw=1 / 32)  # 27 * 256 * 64 < 2^20; eight significand bits hold both exactly


@pytest.mark.parametrize('dtype', [L.DT_BF16, L.DT_F16, L.DT_F32])
@pytest.mark.parametrize('s', [1, 2])
@pytest.mark.parametrize('h,w,cout', [(17, 19, 32), (18, 32, 32), (9, 64, 64)])  # wo % 16 == 0: the MFMA stem
def test_exact_stem(device, h, w, cout, s, dtype):
    """ycx_stem_conv, scalar and MFMA: the fp32 image and weights sit on a grid that the in-kernel
    conversion to the element type keeps unchanged; the output is RNE(true sum)."""
    n, cin, k = 2, 3, 3
    assert 27 * (X_MAX / STEM_GRID['sx']) * (W_MAX / STEM_GRID['sw']) < SPAN
    g = torch.Generator().manual_seed(h * w + s)
    x = dyadic((n, cin, h, w), -X_MAX, X_MAX, STEM_GRID['sx'], g)
    wt = dyadic((cout, cin, k, k), -W_MAX, W_MAX, STEM_GRID['sw'], g)
    b = dyadic((cout,), -B_MAX, B_MAX, B_STEP, g)
    tdt = TDT[dtype]
    for t in (x, wt):
        assert torch.equal(t.to(torch.bfloat16).double(), t) and torch.equal(t.to(torch.float16).double(), t)
    z = F.conv2d(x, wt, b, s, 1)
    ho, wo = z.shape[2:]
    xd, wd, bd = x.float().to(device), wt.permute(2, 3, 1, 0).contiguous().float().to(device), b.float().to(device)
    for act, slope in ACTS:
        ref = apply_act(z, act, slope)
        check_inputs(ref, tdt, "stem")
        d = L.ConvDesc()
        d.n, d.h, d.w, d.cin, d.in_c_off, d.in_c_stride = n, h, w, cin, 0, cin
        d.ho, d.wo, d.cout, d.cout_pad, d.out_c_off, d.out_c_stride = ho, wo, cout, cout, 8, cout + 8
        d.kh = d.kw = k
        d.stride, d.pad, d.act, d.leaky_slope, d.dtype, d.out_layout = s, 1, act, slope, dtype, L.OUT_NHWC
        yd = torch.zeros(n, ho, wo, cout + 8, dtype=tdt, device=device)
        L.check(L.lib.ycx_stem_conv(ctypes.byref(d), xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), yd.data_ptr(),
                                    L.stream_handle(device)))
        torch.cuda.synchronize()
        assert_bits(yd.cpu(), expected(ref, tdt, out_extra=8), f"stem {h}x{w} s{s} dtype {dtype} act {act} {slope}")


def run_stem2(device, dtype, stem_s, act, slope, x, ws, bs, wc, bc, cout):
    """ycx_stem_conv2 on float64 operands (ws [32][3][3][3], wc [cout][32][3][3]); the raw output."""
    n, _, h, w = x.shape
    tdt = TDT[dtype]
    sh, sw = (h - 1) // stem_s + 1, (w - 1) // stem_s + 1
    ho, wo = (sh - 1) // 2 + 1, (sw - 1) // 2 + 1
    ds, dc = L.ConvDesc(), L.ConvDesc()
    ds.n, ds.h, ds.w, ds.cin, ds.in_c_off, ds.in_c_stride = n, h, w, 3, 0, 3
    ds.ho, ds.wo, ds.cout, ds.cout_pad, ds.out_c_off, ds.out_c_stride = sh, sw, 32, 32, 0, 32
    ds.kh = ds.kw = 3
    ds.stride, ds.pad, ds.act, ds.leaky_slope, ds.dtype, ds.out_layout = stem_s, 1, act, slope, dtype, L.OUT_NHWC
    dc.n, dc.h, dc.w, dc.cin, dc.in_c_off, dc.in_c_stride = n, sh, sw, 32, 0, 32
    dc.ho, dc.wo, dc.cout, dc.cout_pad, dc.out_c_off, dc.out_c_stride = ho, wo, cout, 64, 8, cout + 8
    dc.kh = dc.kw = 3
    dc.stride, dc.pad, dc.act, dc.leaky_slope, dc.dtype, dc.out_layout = 2, 1, act, slope, dtype, L.OUT_NHWC
    wcp = torch.zeros(64, 3, 3, 32, dtype=tdt)
    wcp[:cout] = wc.permute(0, 2, 3, 1).to(tdt)
    assert torch.equal(wcp[:cout].double(), wc.permute(0, 2, 3, 1))
    bcp = torch.zeros(64)
    bcp[:cout] = bc.float()
    y = torch.zeros(n, ho, wo, cout + 8, dtype=tdt)
    t = [v.to(device) for v in (x.float(), ws.permute(2, 3, 1, 0).contiguous().float(), bs.float(), wcp, bcp, y)]
    L.check(L.lib.ycx_stem_conv2(ctypes.byref(ds), ctypes.byref(dc), *[v.data_ptr() for v in t],
                                 L.stream_handle(device)))
    torch.cuda.synchronize()
    return t[5].cpu()


@pytest.mark.parametrize('dtype', DT16)
@pytest.mark.parametrize('act,slope', [(L.ACT_NONE, 0.0), (L.ACT_LEAKY, 0.125)])
@pytest.mark.parametrize('stem_s,cout,nhw', [(1, 64, (2, 32, 64)), (2, 48, (2, 64, 128))])
def test_exact_stem2(device, stem_s, cout, nhw, act, slope, dtype):
    """ycx_stem_conv2: the stem map is rounded to the element type as the kernel keeps it in LDS, the
    second conv (w2 in 1/2 steps within +-1) runs on those elements; output bit-exact. The second
    conv's span, 288 * max|mid|/u_mid * 2 < 2^20 with u_mid the stem's unit (x slope under leaky), is
    asserted from the reference. Act none: image and stem weights on the base grid, the bf16 stem map
    needs rounding (|mid| up to ~75 in units of 1/16). Leaky: the slope makes the unit 8 times finer,
    so image and stem weights move to 1/2 steps within +-2 / +-1 (no stem-map rounding there, nor in
    fp16, whose eleven bits hold every stem sum the span bound allows)."""
    n, h, w = nhw
    tdt = TDT[dtype]
    g = torch.Generator().manual_seed(7 + stem_s)
    if act == L.ACT_NONE:  # stem sums in units of 1/16
        x, ws, u = dyadic((n, 3, h, w), -4, 4, 1 / 4, g), dyadic((32, 3, 3, 3), -2, 2, 1 / 4, g), 1 / 16
        bs = dyadic((32,), -B_MAX, B_MAX, 1 / 16, g)
    else:                  # stem sums in units of 1/4, the stem map in units of slope / 4
        x, ws, u = dyadic((n, 3, h, w), -2, 2, 1 / 2, g), dyadic((32, 3, 3, 3), -1, 1, 1 / 2, g), slope / 4
        bs = dyadic((32,), -B_MAX, B_MAX, 1 / 4, g)
    wc = dyadic((cout, 32, 3, 3), -1, 1, 1 / 2, g)
    bc = dyadic((cout,), -B_MAX, B_MAX, B_STEP, g)
    z1 = apply_act(F.conv2d(x, ws, bs, stem_s, 1), act, slope)
    mid = rne(z1, tdt).double()
    assert torch.equal(mid / u, (mid / u).round()) and 288 * float(mid.abs().max()) / u * 2 < SPAN
    if act == L.ACT_NONE and dtype == L.DT_BF16:
        assert rounding_stats(z1, tdt)[0] >= MIN_ROUNDED  # the stem map's rounding is part of the case
    ref = apply_act(F.conv2d(mid, wc, bc, 2, 1), act, slope)
    check_inputs(ref, tdt, "stem2")
    got = run_stem2(device, dtype, stem_s, act, slope, x, ws, bs, wc, bc, cout)
    assert_bits(got, expected(ref, tdt, out_extra=8), f"stem2 s{stem_s} cout {cout} act {act} dtype {dtype}")


@pytest.mark.parametrize('dtype', DT16)
@pytest.mark.parametrize('n,h,w,cin', [(2, 7, 7, 128), (3, 10, 8, 256), (2, 7, 7, 512), (2, 10, 8, 128)])
def test_exact_head_raw_store(device, n, h, w, cin, dtype):
    """ycx_conv2d_head's raw-head store: cout 255 padded to 256, 64-pixel tiles straddling image
    boundaries; conf_thres above 1 appends nothing, and the fp32 NCHW heads are the exact sums."""
    o = operands(dtype, n, h, w, cin, 1, 1)
    tdt, na, nc = TDT[dtype], 3, 80
    cout = na * (nc + 5)
    ref = o.z[:, :cout]
    check_inputs(ref, torch.float32)
    wp = torch.zeros(256, cin, dtype=tdt)
    wp[:cout] = o.wt[:cout, :, 0, 0].to(tdt)
    bp = torch.zeros(256)
    bp[:cout] = o.b[:cout].float()
    d = _desc_1x1(n, h, w, cin, cout, 256, o.in_extra, cin + o.in_extra, 0, cout, L.ACT_NONE, 0.0, dtype)
    d.out_layout = L.OUT_NCHW_F32
    hd = L.HeadDesc()
    rows = na * h * w
    hd.na, hd.no, hd.nc, hd.rows_total, hd.row_off, hd.conf_thres = na, nc + 5, nc, rows, 0, 2.0
    for i in range(2 * na):
        hd.anchors_scaled[i] = 1.0 + i
    xd, wd, bd = o.x_full.to(tdt).to(device), wp.to(device), bp.to(device)
    heads = torch.zeros(n, cout, h, w, device=device)
    cand = torch.zeros(n, rows, 8, device=device)
    cand_rows = torch.zeros(n, rows, dtype=torch.int32, device=device)
    counts = torch.zeros(n, dtype=torch.int32, device=device)
    status = torch.zeros(1, dtype=torch.int32, device=device)
    L.check(L.lib.ycx_conv2d_head(ctypes.byref(d), ctypes.byref(hd), xd.data_ptr(), wd.data_ptr(), bd.data_ptr(),
                                  heads.data_ptr(), cand.data_ptr(), cand_rows.data_ptr(), counts.data_ptr(),
                                  status.data_ptr(), L.stream_handle(device)))
    torch.cuda.synchronize()
    assert not counts.any() and not cand.any() and int(status) == 0
    assert_bits(heads.cpu(), ref.float(), f"head cin {cin} {h}x{w} dtype {dtype}")


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


def check_silu(got, z, act, tdt, what, out_extra=16):
    """got: the raw NHWC output buffer; z: the exact pre-activation NCHW (of the packed operands).
    Elements are compared as values: +0 and -0 (silu(0) of either sign) coincide."""
    ref, excused, sub, share = silu_conditions(z, act, tdt, what)
    assert not got[..., :out_extra].any(), "wrote outside the output channel slice"
    g = got[..., out_extra:].contiguous()
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


SILU_CASES = [(3, 2, 13, 11, 64, 64, 3, 1, 0), (16, 2, 13, 11, 64, 128, 3, 1, 0), (18, 2, 13, 11, 64, 64, 3, 1, 0),
              (20, 2, 16, 16, 64, 128, 3, 1, 0), (22, 2, 13, 11, 64, 64, 1, 1, 0), (23, 2, 16, 16, 64, 64, 3, 1, 0),
              (50, 2, 32, 64, 64, 128, 3, 2, 0), (16, 2, 13, 11, 256, 128, 1, 1, 2)]  # last: the split-K reduce


@pytest.mark.parametrize('act', [L.ACT_SILU, L.ACT_SILU_PS])
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


@pytest.mark.parametrize('act', [L.ACT_SILU, L.ACT_SILU_PS])
@pytest.mark.parametrize('dtype', DT16)
def test_silu_ulps_stem2(device, dtype, act):
    """stem2's two SiLU epilogues: the stem map must be RNE(silu) (any other element moves z2 by far
    more than an ulp), the output is held to the ulp bar."""
    x, ws, bs, wc, bc, z2 = stem2_silu_operands(act, dtype)
    got = run_stem2(device, dtype, 1, act, 0.0, x, ws, bs, wc, bc, 64)
    check_silu(got, z2, act, TDT[dtype], f"stem2 dtype {dtype} act {act}", out_extra=8)
