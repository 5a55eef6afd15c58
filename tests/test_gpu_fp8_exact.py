"""Bit-exact e4m3 stores on exactly representable operands ("exact-operand bar", fp8).

The method of tests/test_gpu_conv_exact.py on the kernels that run on, or store, OCP e4m3fn. Every
operand is a small dyadic rational that IS an e4m3 value (at most four significant bits, asserted by
a round trip through torch.float8_e4m3fn), every scale is a power of two and the block-scaled MFMA
accumulates in fp32, so every product and partial sum is exact under the span bound
K * max|x|/step_x * max|w|/step_w < 2^20, and so is each epilogue step (ycx_conv.hip: epilogue_f8,
epilogue_f8x8, store4_f8, store8_f8, f8_sat, f8x4_pack): fma(acc, dq, bias), leaky with a
power-of-two slope, + residual * res_scale, * out_scale. The stored byte must equal torch's e4m3fn
cast (round to nearest even; tests/test_gpu_fp8.py::test_quantize_matches_torch_cast pins it as the
encoding) of the float64 reference clamped to +-448: no tolerance, whole buffers compared.

Operands (real values; stored bytes are e4m3(x * s_x), e4m3(w * s_w[co])):
  x in 1/4 steps within +-4, w in 1/4 steps within +-2, bias in 1/16 steps within +-2; s_x = 8;
  s_w[co] = 2^((co + co/4 + co/16 + co/64) % 4) (integer divisions), so dq[co] = 1 / (s_w[co] s_x) takes
  four values in every aligned 4-channel group and differs between co and co + 2^j, j = 0 .. 5, for at
  least half of the channels: an epilogue that reads dq one, four, eight or 32 channels off shows; bias is
  [2 cout_pad] (bias, then dq).
  Weight rows are [cout_pad][ceil(K / 128) * 128]. The row padding is ZERO: ycx.h and the kernel
  header make that the caller's contract ("the tail step adds exact zeros"; tile 37's tenth tap), so
  it is a precondition here, not something tested. Every channel, the padded ones cout ..< cout_pad
  included, has a nonzero weight row, bias (a zero draw becomes 1/16) and dq, all asserted, so a store
  past cout shows.
Output buffers are wider than the written slice on both sides and pre-filled with a sentinel byte
(fp32 NCHW: a sentinel float and a channel on either side).

Two output scales per case, chosen from the float64 reference alone (out_scales):
  so_hi  the smallest power of two at which >= 0.5 % of |ref * so| exceed 448 (asserted <= 20 %):
         the +-448 clamp is part of every case;
  so_lo  the largest power of two <= so_hi / 64 (and >= so_hi / 512) at which >= 0.1 % of the outputs
         are nonzero with |ref * so| < 2^-6, e4m3's subnormal range.
Input conditions, asserted per case and scale from the reference alone (tests/test_fp8_exact_plan.py
walks the same table without a GPU): among the outputs the clamp leaves alone >= 10 % are not e4m3
values and >= 1 % are exact ties.

kernel -> cases (act none and leaky 0.125 each):
  tiles 34, 35       test_exact_f8_general: n 2, 13 x 11, in_extra 16; (cin, k, s) = (32,3,2) (64,3,1)
                     (128,3,1) (256,1,1): TPS 4, 2, 1, 1; (96,3,1) (48,3,2) (160,1,1): the generic K walk
                     (chunks cross taps, partial last K step); tile 34 cout_pad 128, tile 35 cout 64 / 192
                     test_exact_f8_variants: residual (e4m3 bytes of their own grid and scale), x2
                     upsample, fp32 NCHW (cout 255 of 256, unscaled: the exact sum as int32 bits),
                     cout 120 of 128, in_pool at cin 128 and 256 (the pooled bytes are exact)
  tile 36            test_exact_f8_wres: cin 128 / 256 / 512 x cout_pad 64 / 128 / 256 and 248 of 256 at 13 x 11
                     (one tile per block, more ranges than tiles); n 2, 96 x 96 at cout_pad 256 / 512 and n 2,
                     184 x 180 at cout_pad 64 / 128: two or three tiles per block (the deferred epilogue), at
                     cin 512 more ring steps than stages (the ring wraps; 248 of 256 too), and at three tiles
                     per block waits counted against store batches in flight, on each of the three launch
                     shapes. wres_plan restates the launch arithmetic and each case asserts what it reaches.
  tile 37            test_exact_f8_ws64: 16 x 16 and 32 x 48, cout 64 and 48 (halo zeros, the zero tenth tap)
  tile 39 (head)     test_exact_f8_head: cin 128 / 256 / 512 on 7 x 7 and 10 x 8, conf_thres 2: no candidates,
                     status 0, the fp32 heads are the exact acc * dq + bias
  ycx_stem_conv      test_exact_f8_stem_store: test_exact_stem's three shapes, s 1 and 2 (fp32 / bf16
                     compute, one rounding fp32 -> e4m3); image and weights on the base grid, since the
                     16-bit test's 1/64 x 1/32 grid leaves e4m3 almost no ties
  ycx_stem_conv2     test_exact_f8_stem2_store: test_exact_stem2's two shapes, both descriptors fp8; the
                     reference rounds the stem map to bf16 as the kernel keeps it; a coarse grid on both
                     shapes and a finer one on the first (STEM2_GRID)
  ycx_copy_channels  test_f8_copy_channels: all 254 finite codes, scale 1 and 2, both channel slices,
                     fp32 NCHW with a power-of-two dequant as int32 bits
  SiLU, SILU_PS      test_f8_silu_ulps (tiles 35, 36, 37), test_f8_silu_ulps_stem2: the ulp bar of
                     test_silu_ulps, below
"""
import ctypes
import functools
import math
import types

import pytest
import torch
import torch.nn.functional as F

from helpers import E4M3, dyadic, e4m3_is_nan, elt_neighbours, elt_ulps, rne, rounding_stats
from test_gpu_conv_exact import B_MAX, B_STEP, SILU_MAX_Z, SPAN, W_MAX, X_MAX, apply_act, silu_ref, stem2_silu_operands

pytestmark = pytest.mark.gpu

L = pytest.importorskip("ycx._lib")

ACTS = [(L.ACT_NONE, 0.0), (L.ACT_LEAKY, 0.125)]
MIN_ROUNDED, MIN_TIES = 0.10, 0.01
MIN_SAT, MAX_SAT, MIN_SUB = 0.005, 0.20, 0.001
MAX_EXCUSED = 0.001          # e4m3 boundaries are 2^-4 apart relatively: ~1e-4 of the elements at these margins
F8_MAX, F8_MIN_NORMAL = 448.0, 2.0 ** -6
S_X = 8.0
SENT = 0x5A                  # sentinel byte of the output buffers (a finite e4m3 code, never zero)
SENT_F32 = 12345.0
IN_EXTRA, OUT_EXTRA, OUT_TAIL = 16, 16, 8
X_STEP = W_STEP = 1 / 4


def is_e4m3(t64):
    return torch.equal(t64.to(E4M3).double(), t64)


def q8(ref64, so):
    """The expected bytes: torch's e4m3fn cast of clamp(ref * so, +-448)."""
    return rne((ref64 * so).clamp(-F8_MAX, F8_MAX), E4M3).view(torch.uint8)


def scale_stats(ref64, so):
    """(rounded, ties) among the outputs the clamp leaves alone, the saturated share and the share of
    nonzero outputs in the subnormal range, of ref * so."""
    v = (ref64 * so).reshape(-1)
    a = v.abs()
    rounded, ties = rounding_stats(v[a <= F8_MAX], E4M3)
    return rounded, ties, float((a > F8_MAX).double().mean()), float(((a > 0) & (a < F8_MIN_NORMAL)).double().mean())


def out_scales(ref64, what=""):
    """(so_hi, so_lo) of the module docstring and the conditions of both, from the reference alone.
    Returns (so_hi, so_lo, stats) with stats = {so: (rounded, ties, saturated, subnormal)}."""
    a = ref64.abs().reshape(-1)
    e_hi = next(e for e in range(-16, 17) if float((a * 2.0 ** e > F8_MAX).double().mean()) >= MIN_SAT)
    e_lo = next((e for e in range(e_hi - 6, e_hi - 10, -1)
                 if float(((a > 0) & (a * 2.0 ** e < F8_MIN_NORMAL)).double().mean()) >= MIN_SUB), None)
    assert e_lo is not None, f"{what}: no scale within so_hi / 512 puts {MIN_SUB} of the outputs in the subnormal range"
    so_hi, so_lo = 2.0 ** e_hi, 2.0 ** e_lo
    stats = {so: scale_stats(ref64, so) for so in (so_hi, so_lo)}
    for so, (rounded, ties, sat, sub) in stats.items():
        assert rounded >= MIN_ROUNDED and ties >= MIN_TIES, \
            f"{what} so {so}: inputs too easy, {rounded:.3f} of the outputs need rounding, {ties:.3f} are ties"
    assert MIN_SAT <= stats[so_hi][2] <= MAX_SAT, f"{what}: {stats[so_hi][2]:.4f} saturate at so_hi {so_hi}"
    assert stats[so_lo][3] >= MIN_SUB and stats[so_lo][2] == 0.0, f"{what}: {stats[so_lo]} at so_lo {so_lo}"
    return so_hi, so_lo, stats


def assert_bytes(got, exp, what=""):
    """torch.equal on whole uint8 buffers; on a mismatch, say how many bytes and how far (NaN codes apart)."""
    assert got.dtype == torch.uint8 and exp.dtype == torch.uint8 and got.shape == exp.shape, what
    if torch.equal(got, exp):
        return
    bad = got != exp
    nan = int((e4m3_is_nan(got) & bad).sum())
    d = elt_ulps(got.view(E4M3), exp.view(E4M3), E4M3)[bad]
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} bytes differ from e4m3(clamp(ref * so)); "
                         f"{nan} are NaN codes; distance in codes: min {int(d.min())}, max {int(d.max())}; "
                         f"first at {[int(v) for v in bad.nonzero()[0]]}")


def assert_f32_bits(got, exp, what=""):
    assert got.dtype == torch.float32 and exp.dtype == torch.float32 and got.shape == exp.shape, what
    bad = got.contiguous().view(torch.int32) != exp.contiguous().view(torch.int32)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} fp32 values differ from the exact sum; " \
                          f"first at {[int(v) for v in bad.nonzero()[0]]}"


def framed(ref_nhwc_bytes, lead=OUT_EXTRA, tail=OUT_TAIL):
    """The whole expected buffer: the slice between ``lead`` and ``tail`` sentinel channels."""
    exp = torch.full((*ref_nhwc_bytes.shape[:3], lead + ref_nhwc_bytes.shape[3] + tail), SENT, dtype=torch.uint8)
    exp[..., lead:lead + ref_nhwc_bytes.shape[3]] = ref_nhwc_bytes
    return exp


# ---- the fp8 convs (ycx_conv2d tiles 34-37, ycx_conv2d_head tile 39) ----
@functools.lru_cache(maxsize=4)  # consecutive cases share operands; the large tile-36 maps are not kept
def operands(n, h, w, cin, k, s, cpad, pool=False, seed=0, grid=None):
    """Operands of one conv, shared by every tile / act / scale / variant that runs it, never modified:
    x_full [n][h][w][IN_EXTRA + cin] NHWC, wt [cpad][cin][k][k], b [cpad] (float64; every channel, padded
    ones included, has a nonzero bias, a nonzero weight row and a nonzero dq), s_w [cpad], the packed e4m3
    bytes xq / wq, the fp32 [2 cpad] bias row and the exact pre-activation z [n][cpad][ho][wo].
    pool: x_full is the (2h, 2w) map of the fused max-pool.
    grid: (step_x, step_w, max|x|, max|w|) where a case needs another than the base grid."""
    sx, sw, xm, wm = grid or (X_STEP, W_STEP, X_MAX, W_MAX)
    K = cin * k * k
    assert K * (xm / sx) * (wm / sw) < SPAN and K <= 8191
    g = torch.Generator().manual_seed(1000 * seed + 17 * cin + k + s + 7)
    up = 2 if pool else 1
    o = types.SimpleNamespace(n=n, h=h, w=w, cin=cin, k=k, s=s, cpad=cpad, pool=pool)
    o.x_full = dyadic((n, up * h, up * w, IN_EXTRA + cin), -xm, xm, sx, g)
    o.wt = dyadic((cpad, cin, k, k), -wm, wm, sw, g)
    o.b = dyadic((cpad,), -B_MAX, B_MAX, B_STEP, g)
    o.b[o.b == 0] = B_STEP                       # no zero bias: a padded channel that is stored shows
    co = torch.arange(cpad)
    o.s_w = 2.0 ** ((co + co // 4 + co // 16 + co // 64) % 4).double()
    xs, ws = o.x_full * S_X, o.wt * o.s_w.reshape(-1, 1, 1, 1)
    for t in (o.x_full, o.wt, xs, ws):           # every MFMA operand is an e4m3 value, scaled or not
        assert is_e4m3(t)
    for t in (xs, ws):                           # the stored bytes are normal and inside the range
        assert float(t.abs().max()) <= F8_MAX and float(t[t != 0].abs().min()) >= F8_MIN_NORMAL
    assert all(len(set(o.s_w[i:i + 4].tolist())) == 4 for i in range(0, cpad, 4))
    assert all(float((o.s_w != o.s_w.roll(-(1 << j)))[:cpad - (1 << j)].double().mean()) >= 0.5 for j in range(6))
    o.xq = xs.to(E4M3).view(torch.uint8)
    kp = -(-K // 128) * 128
    o.wq = torch.zeros(cpad, kp, dtype=torch.uint8)                 # row padding: zero (precondition)
    o.wq[:, :K] = ws.permute(0, 2, 3, 1).reshape(cpad, K).to(E4M3).view(torch.uint8)
    o.bias = torch.cat([o.b, 1.0 / (o.s_w * S_X)]).float()
    assert bool(o.wq.any(1).all() and (o.bias != 0).all())  # padded channels too: nonzero rows, bias and dq
    x = o.x_full[..., IN_EXTRA:].permute(0, 3, 1, 2)
    if pool:
        x = F.max_pool2d(x, 2, 2)  # exact
    if k == 1 and s == 1:  # the same float64 sums as one matrix product (the large tile-36 maps)
        o.z = (torch.einsum('nchw,oc->nohw', x, o.wt[:, :, 0, 0]) + o.b.reshape(1, -1, 1, 1)).contiguous()
    else:
        o.z = F.conv2d(x, o.wt, o.b, s, k // 2)
    o.ho, o.wo = o.z.shape[2:]
    return o


RES_S = 4.0  # the residual's own scale: bytes e4m3(r * 4), res_scale 1/4


def residual_of(o, cout, seed):
    """Residual on a grid of its own: 1/2 steps within +-4 (e4m3 values, scaled by 4 too)."""
    r = dyadic((o.n, o.ho, o.wo, cout), -4, 4, 1 / 2, torch.Generator().manual_seed(seed))
    assert is_e4m3(r) and is_e4m3(r * RES_S)
    return r


def conv_desc(o, tile, cout, act, slope, so, layout, lead, stride_c):
    d = L.ConvDesc()
    d.n, d.h, d.w, d.cin, d.in_c_off, d.in_c_stride = o.n, o.h, o.w, o.cin, IN_EXTRA, o.cin + IN_EXTRA
    d.ho, d.wo, d.cout, d.cout_pad, d.out_c_off, d.out_c_stride = o.ho, o.wo, cout, o.cpad, lead, stride_c
    d.kh = d.kw = o.k
    d.stride, d.pad, d.act, d.leaky_slope = o.s, 0 if o.pool else o.k // 2, act, slope
    d.dtype, d.out_layout, d.tile, d.in_pool = L.DT_FP8, layout, tile, int(o.pool)
    d.out_scale, d.res_scale = so, 1.0 / RES_S
    return d


def launch(device, o, tile, cout, act, slope, so, layout=L.OUT_NHWC, residual=None, bias=None):
    """One ycx_conv2d on operands ``o`` (first ``cout`` channels); the raw output buffer."""
    up = 2 if layout == L.OUT_NHWC_UP2 else 1
    if layout == L.OUT_NCHW_F32:
        y = torch.full((o.n, cout + 2, o.ho, o.wo), SENT_F32, dtype=torch.float32)
        d = conv_desc(o, tile, cout, act, slope, 1.0, layout, 1, cout + 2)
    else:
        y = torch.full((o.n, o.ho * up, o.wo * up, OUT_EXTRA + cout + OUT_TAIL), SENT, dtype=torch.uint8)
        d = conv_desc(o, tile, cout, act, slope, so, layout, OUT_EXTRA, OUT_EXTRA + cout + OUT_TAIL)
    rd = None
    if residual is not None:  # its own buffer, slice at 8 of cout + 8
        rb = torch.full((o.n, o.ho, o.wo, 8 + cout), SENT, dtype=torch.uint8)
        rb[..., 8:] = (residual * RES_S).to(E4M3).view(torch.uint8)
        d.res_c_off, d.res_c_stride = 8, cout + 8
        rd = rb.to(device)
    xd, wd, yd = o.xq.to(device), o.wq.to(device), y.to(device)
    bd = (o.bias if bias is None else bias).to(device)
    L.check(L.lib.ycx_conv2d(ctypes.byref(d), xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), yd.data_ptr(), L.ptr(rd),
                             L.stream_handle(device)), "fp8 conv")
    torch.cuda.synchronize()
    return yd.cpu()


def conv_refs(o, cout, variant=None, seed=0):
    """(act, slope, residual, float64 reference NCHW) per act of one conv case."""
    for act, slope in ACTS:
        ref = apply_act(o.z[:, :cout], act, slope)
        r = None
        if variant == 'residual':
            r = residual_of(o, cout, seed)
            ref = ref + r.permute(0, 3, 1, 2)
        yield act, slope, r, ref


def run_conv(device, o, tile, cout, what, variant=None):
    """Both acts x both output scales of one conv case, whole buffers bit for bit."""
    layout = {'up2': L.OUT_NHWC_UP2, 'nchw_f32': L.OUT_NCHW_F32}.get(variant, L.OUT_NHWC)
    for act, slope, r, ref in conv_refs(o, cout, variant, tile):
        w_ = f"{what} act {act}"
        if layout == L.OUT_NCHW_F32:  # unscaled: the exact sum
            assert torch.equal(ref.float().double(), ref)
            exp = torch.full((o.n, cout + 2, o.ho, o.wo), SENT_F32)
            exp[:, 1:cout + 1] = ref.float()
            assert_f32_bits(launch(device, o, tile, cout, act, slope, 1.0, layout), exp, w_)
            continue
        so_hi, so_lo, _ = out_scales(ref, w_)
        for so in (so_hi, so_lo):
            eb = q8(ref.permute(0, 2, 3, 1), so)
            if layout == L.OUT_NHWC_UP2:
                eb = eb.repeat_interleave(2, 1).repeat_interleave(2, 2)
            assert_bytes(launch(device, o, tile, cout, act, slope, so, layout, r), framed(eb), f"{w_} so {so}")


CKS = [(32, 3, 2), (64, 3, 1), (128, 3, 1), (256, 1, 1), (96, 3, 1), (48, 3, 2), (160, 1, 1)]
GENERAL = [(34, 128, 128), (35, 64, 64), (35, 192, 192)]  # tile, cout, cout_pad
VARIANTS = ['residual', 'up2', 'nchw_f32', 'cout_below_pad', 'in_pool_128', 'in_pool_256']
# h, w, cin, cout, cout_pad, what wres_plan must report: '' one tile per block, 'm' several tiles on some block
# (the deferred epilogue), 'w' more ring steps than stages on some block (the ring wraps onto a used stage),
# 'c' a wait counted against store batches in flight (wait_vm_counted with nb > 0)
WRES = ([(13, 11, cin, cp, cp, '') for cin in (128, 256, 512) for cp in (64, 128, 256)] +
        [(13, 11, 256, 248, 256, ''), (96, 96, 128, 256, 256, 'm'), (96, 96, 512, 256, 256, 'mw'),
         (96, 96, 512, 248, 256, 'mw'), (96, 96, 512, 512, 512, 'mwc'), (184, 180, 512, 64, 64, 'mwc'),
         (184, 180, 512, 128, 128, 'mwc')])


def wres_plan(m, cin, cout, cpad):
    """What a tile-36 launch of m pixels does, restated from launch_wres_f8 / launch_wres_f8_k / conv1x1_wres_f8
    (ycx_conv.hip): the launch shape (WCO, WPX, TPW, NS) by cout_pad, PT = TPW WPX pixels per tile, KC = cin / 128
    ring steps per tile, R = even_grid(T, 256 / n_ct) persistent blocks per channel group, block r owning tiles
    [r T / R, (r + 1) T / R), and the wait taken before ring step t of a block's nst = tiles KC steps. Returns
    the flags of WRES."""
    wco, wpx, tpw, ns = (8, 1, 64, 5) if cpad % 256 == 0 else (4, 2, 64, 6) if cpad == 128 else (2, 4, 32, 6)
    pt, kc, n_ct = tpw * wpx, cin // 128, cpad // (wco * 32)
    T, cap = -(-m // pt), 256 // n_ct
    R = T if T <= cap else -(-T // -(-T // cap))
    flags = set()
    for r in range(R):
        nst = ((r + 1) * T // R - r * T // R) * kc
        if nst > kc:
            flags.add('m')
        if nst > ns:
            flags.add('w')
        for t in range(nst):
            if t + ns - 2 >= nst:  # the tail: vmcnt(0)
                continue
            lo = max(t - ns + 1, kc)
            if cout == cpad and t - 1 >= lo and (t - 1) // kc - (lo + kc - 1) // kc + 1 > 0:
                flags.add('c')
    return ''.join(f for f in 'mwc' if f in flags)


WS64 = [(16, 16, 64), (32, 48, 64), (16, 16, 48), (32, 48, 48)]  # h, w, cout
HEADS = [(2, 7, 7, 128), (3, 10, 8, 256), (2, 7, 7, 512), (2, 10, 8, 128), (2, 10, 8, 512), (2, 7, 7, 256)]


def variant_case(tile, variant):
    """(operands, cout) of one variant on tile 34 / 35 (cout_pad 128 or 256)."""
    if variant.startswith('in_pool'):
        return operands(2, 13, 11, int(variant[8:]), 1, 1, 128, pool=True), 128
    if variant == 'nchw_f32':
        return operands(2, 13, 11, 64, 3, 1, 256), 255
    return operands(2, 13, 11, 64, 3, 1, 128), 120 if variant == 'cout_below_pad' else 128


@pytest.mark.parametrize('cin,k,s', CKS)
@pytest.mark.parametrize('tile,cout,cpad', GENERAL)
def test_exact_f8_general(device, tile, cout, cpad, cin, k, s):
    """Tiles 34 / 35 on every K walk: ragged pixel tail, image borders, both channel slices."""
    run_conv(device, operands(2, 13, 11, cin, k, s, cpad), tile, cout, f"tile {tile} cout {cout} cin {cin} k{k} s{s}")


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('tile', [34, 35])
def test_exact_f8_variants(device, tile, variant):
    """The other stores of epilogue_f8 / epilogue_f8x8 / store4_f8 / store8_f8 and the pooled operand."""
    o, cout = variant_case(tile, variant)
    run_conv(device, o, tile, cout, f"tile {tile} {variant}", variant)


@pytest.mark.parametrize('h,w,cin,cout,cpad,plan', WRES)
def test_exact_f8_wres(device, h, w, cin, cout, cpad, plan):
    """Tile 36: its three launch shapes at every resident K and cout < cout_pad on one tile per block; then
    several tiles per block (the deferred epilogue), with and without cout < cout_pad, the ring wrapping onto
    used stages, and the store-counted waits, on each launch shape (wres_plan asserts which case reaches what)."""
    assert wres_plan(2 * h * w, cin, cout, cpad) == plan
    run_conv(device, operands(2, h, w, cin, 1, 1, cpad), 36, cout, f"tile 36 {h}x{w} cin {cin} cout {cout}/{cpad}")


@pytest.mark.parametrize('h,w,cout', WS64)
def test_exact_f8_ws64(device, h, w, cout):
    """Tile 37: image borders are the halo's zeros, the tenth tap is the (zero) row padding."""
    run_conv(device, operands(2, h, w, 64, 3, 1, 64), 37, cout, f"tile 37 {h}x{w} cout {cout}")


@pytest.mark.parametrize('n,h,w,cin', HEADS)
def test_exact_f8_head(device, n, h, w, cin):
    """ycx_conv2d_head in fp8 (tile 39), as test_exact_head_raw_store: cout 255 of 256, 64-pixel tiles
    straddling images; conf_thres above 1 appends nothing; the fp32 NCHW heads are acc * dq + bias exactly."""
    o = operands(n, h, w, cin, 1, 1, 256)
    na, nc = 3, 80
    cout = na * (nc + 5)
    ref = o.z[:, :cout]
    assert torch.equal(ref.float().double(), ref)
    d = conv_desc(o, 0, cout, L.ACT_NONE, 0.0, 1.0, L.OUT_NCHW_F32, 0, cout)
    hd = L.HeadDesc()
    rows = na * h * w
    hd.na, hd.no, hd.nc, hd.rows_total, hd.row_off, hd.conf_thres = na, nc + 5, nc, rows, 0, 2.0
    for i in range(2 * na):
        hd.anchors_scaled[i] = 1.0 + i
    xd, wd, bd = o.xq.to(device), o.wq.to(device), o.bias.to(device)
    heads = torch.full((n, cout, h, w), SENT_F32, device=device)
    cand = torch.zeros(n, rows, 8, device=device)
    cand_rows = torch.zeros(n, rows, dtype=torch.int32, device=device)
    counts = torch.zeros(n, dtype=torch.int32, device=device)
    status = torch.zeros(1, dtype=torch.int32, device=device)
    L.check(L.lib.ycx_conv2d_head(ctypes.byref(d), ctypes.byref(hd), xd.data_ptr(), wd.data_ptr(), bd.data_ptr(),
                                  heads.data_ptr(), cand.data_ptr(), cand_rows.data_ptr(), counts.data_ptr(),
                                  status.data_ptr(), L.stream_handle(device)))
    torch.cuda.synchronize()
    assert not counts.any() and not cand.any() and int(status) == 0
    assert_f32_bits(heads.cpu(), ref.float(), f"fp8 head cin {cin} {h}x{w}")


# ---- e4m3 stores of the kernels that compute in fp32 / bf16 ----
STEM_SHAPES = [(17, 19, 32), (18, 32, 32), (9, 64, 64)]  # test_exact_stem's; wo % 16 == 0: the MFMA stem
# ycx_stem_conv2, per grid and act: (image step, max), (stem w step, max), stem bias step, (w2 step, max), b2 step.
# Coarser than test_exact_stem2's, whose sums carry so many low bits that e4m3 would see almost no ties; the stem
# map is still rounded to bf16 in the reference, as the kernel keeps it. 'coarse' runs on both shapes; 'fine'
# (quarter / half steps, five w2 values: many more distinct sums, ties still 2.7-4.3 %) on the first.
STEM2_GRID = {('coarse', L.ACT_NONE): ((1.0, 2.0), (1 / 2, 1.0), 1 / 2, (1.0, 1.0), 1 / 2),
              ('coarse', L.ACT_LEAKY): ((1.0, 2.0), (1.0, 1.0), 1.0, (1.0, 1.0), 1 / 8),
              ('fine', L.ACT_NONE): ((1 / 4, 2.0), (1 / 2, 1.0), 1 / 8, (1 / 2, 1.0), 1 / 8),
              ('fine', L.ACT_LEAKY): ((1 / 2, 2.0), (1.0, 1.0), 1 / 2, (1 / 2, 1.0), 1 / 8)}
STEM2_SHAPES = [(1, 64, (2, 32, 64), 'coarse'), (2, 48, (2, 64, 128), 'coarse'),  # test_exact_stem2's shapes
                (1, 64, (2, 32, 64), 'fine')]


@functools.lru_cache(maxsize=None)
def stem_operands(h, w, cout, s):
    """Image [2][3][h][w] and weights [cout][3][3][3] on the base grid (exact in bf16 too), bias; the exact z."""
    assert 27 * (X_MAX / X_STEP) * (W_MAX / W_STEP) < SPAN
    g = torch.Generator().manual_seed(h * w + s)
    o = types.SimpleNamespace(h=h, w=w, cout=cout, s=s)
    o.x = dyadic((2, 3, h, w), -X_MAX, X_MAX, X_STEP, g)
    o.wt = dyadic((cout, 3, 3, 3), -W_MAX, W_MAX, W_STEP, g)
    o.b = dyadic((cout,), -B_MAX, B_MAX, B_STEP, g)
    for t in (o.x, o.wt):
        assert torch.equal(t.to(torch.bfloat16).double(), t)
    o.z = F.conv2d(o.x, o.wt, o.b, s, 1)
    return o


@pytest.mark.parametrize('s', [1, 2])
@pytest.mark.parametrize('h,w,cout', STEM_SHAPES)
def test_exact_f8_stem_store(device, h, w, cout, s):
    """ycx_stem_conv with dtype fp8, scalar and MFMA stems: the fp32 value is cast straight to e4m3."""
    o = stem_operands(h, w, cout, s)
    n, (ho, wo) = 2, o.z.shape[2:]
    xd, wd, bd = [t.float().to(device) for t in (o.x, o.wt.permute(2, 3, 1, 0).contiguous(), o.b)]
    for act, slope in ACTS:
        ref = apply_act(o.z, act, slope)
        what = f"stem {h}x{w} s{s} act {act}"
        so_hi, so_lo, _ = out_scales(ref, what)
        for so in (so_hi, so_lo):
            d = L.ConvDesc()
            d.n, d.h, d.w, d.cin, d.in_c_off, d.in_c_stride = n, h, w, 3, 0, 3
            d.ho, d.wo, d.cout, d.cout_pad, d.out_c_off, d.out_c_stride = ho, wo, cout, cout, 8, cout + 16
            d.kh = d.kw = 3
            d.stride, d.pad, d.act, d.leaky_slope, d.dtype, d.out_layout = s, 1, act, slope, L.DT_FP8, L.OUT_NHWC
            d.out_scale = so
            yd = torch.full((n, ho, wo, cout + 16), SENT, dtype=torch.uint8, device=device)
            L.check(L.lib.ycx_stem_conv(ctypes.byref(d), xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), yd.data_ptr(),
                                        L.stream_handle(device)))
            torch.cuda.synchronize()
            assert_bytes(yd.cpu(), framed(q8(ref.permute(0, 2, 3, 1), so), 8, 8), f"{what} so {so}")


def run_stem2_f8(device, stem_s, act, slope, so, x, ws, bs, wc, bc, cout):
    """ycx_stem_conv2 with both descriptors fp8 (bf16 compute, bf16 w_conv, plain bias); the raw output."""
    n, _, h, w = x.shape
    sh, sw = (h - 1) // stem_s + 1, (w - 1) // stem_s + 1
    ho, wo = (sh - 1) // 2 + 1, (sw - 1) // 2 + 1
    ds, dc = L.ConvDesc(), L.ConvDesc()
    ds.n, ds.h, ds.w, ds.cin, ds.in_c_off, ds.in_c_stride = n, h, w, 3, 0, 3
    ds.ho, ds.wo, ds.cout, ds.cout_pad, ds.out_c_off, ds.out_c_stride = sh, sw, 32, 32, 0, 32
    ds.kh = ds.kw = 3
    ds.stride, ds.pad, ds.act, ds.leaky_slope, ds.dtype, ds.out_layout = stem_s, 1, act, slope, L.DT_FP8, L.OUT_NHWC
    dc.n, dc.h, dc.w, dc.cin, dc.in_c_off, dc.in_c_stride = n, sh, sw, 32, 0, 32
    dc.ho, dc.wo, dc.cout, dc.cout_pad, dc.out_c_off, dc.out_c_stride = ho, wo, cout, 64, 8, cout + 16
    dc.kh = dc.kw = 3
    dc.stride, dc.pad, dc.act, dc.leaky_slope, dc.dtype, dc.out_layout = 2, 1, act, slope, L.DT_FP8, L.OUT_NHWC
    dc.out_scale = ds.out_scale = so
    wcp = torch.zeros(64, 3, 3, 32, dtype=torch.bfloat16)
    wcp[:cout] = wc.permute(0, 2, 3, 1).to(torch.bfloat16)
    wcp[cout:] = 1.0                      # padded output channels: nonzero weights and bias
    assert torch.equal(wcp[:cout].double(), wc.permute(0, 2, 3, 1))
    bcp = torch.ones(64)
    bcp[:cout] = bc.float()
    y = torch.full((n, ho, wo, cout + 16), SENT, dtype=torch.uint8)
    t = [v.to(device) for v in (x.float(), ws.permute(2, 3, 1, 0).contiguous().float(), bs.float(), wcp, bcp, y)]
    L.check(L.lib.ycx_stem_conv2(ctypes.byref(ds), ctypes.byref(dc), *[v.data_ptr() for v in t],
                                 L.stream_handle(device)))
    torch.cuda.synchronize()
    return t[5].cpu()


@functools.lru_cache(maxsize=None)
def stem2_operands(stem_s, cout, nhw, act, slope, grid='coarse'):
    """Operands of one ycx_stem_conv2 case on STEM2_GRID[grid, act] and its float64 reference: the stem map
    rounded to bf16, then the second conv on those elements. The second conv's span bound,
    288 * max|mid|/u_mid * max|w2|/step_w2 < 2^20, is asserted from the reference."""
    (sx, xm), (sw, wm), sb, (s2, w2m), sb2 = STEM2_GRID[grid, act]
    n, h, w = nhw
    g = torch.Generator().manual_seed(7 + stem_s)
    x, ws, bs = dyadic((n, 3, h, w), -xm, xm, sx, g), dyadic((32, 3, 3, 3), -wm, wm, sw, g), dyadic((32,), -2, 2, sb, g)
    wc, bc = dyadic((cout, 32, 3, 3), -w2m, w2m, s2, g), dyadic((cout,), -B_MAX, B_MAX, sb2, g)
    for t in (x, ws, wc):
        assert torch.equal(t.to(torch.bfloat16).double(), t)
    u = min(sx * sw, sb) * (slope if act == L.ACT_LEAKY else 1.0)
    assert 27 * (xm / sx) * (wm / sw) < SPAN
    mid = rne(apply_act(F.conv2d(x, ws, bs, stem_s, 1), act, slope), torch.bfloat16).double()
    assert torch.equal(mid / u, (mid / u).round()) and 288 * float(mid.abs().max()) / u * (w2m / s2) < SPAN
    ref = apply_act(F.conv2d(mid, wc, bc, 2, 1), act, slope)
    return x, ws, bs, wc, bc, ref


@pytest.mark.parametrize('act,slope', ACTS)
@pytest.mark.parametrize('stem_s,cout,nhw,grid', STEM2_SHAPES)
def test_exact_f8_stem2_store(device, stem_s, cout, nhw, grid, act, slope):
    """ycx_stem_conv2 with both descriptors fp8: bf16 compute as in test_exact_stem2, the output one
    rounding fp32 -> e4m3 of the exact second sum."""
    x, ws, bs, wc, bc, ref = stem2_operands(stem_s, cout, nhw, act, slope, grid)
    what = f"stem2 s{stem_s} cout {cout} {grid} act {act}"
    so_hi, so_lo, _ = out_scales(ref, what)
    for so in (so_hi, so_lo):
        got = run_stem2_f8(device, stem_s, act, slope, so, x, ws, bs, wc, bc, cout)
        assert_bytes(got, framed(q8(ref.permute(0, 2, 3, 1), so), 8, 8), f"{what} so {so}")


# ---- ycx_copy_channels in fp8 ----
def copy_input(n=2, h=5, w=7, c=24, lead=8, tail=16):
    """Bytes [n][h][w][lead + c + tail] that hold each of the 254 finite e4m3 codes inside the channel
    slice (a fixed permutation, then seeded draws); the slice bounds."""
    finite = torch.tensor([b for b in range(256) if b & 0x7F != 0x7F], dtype=torch.uint8)
    g = torch.Generator().manual_seed(254)
    x = finite[torch.randint(0, 254, (n, h, w, lead + c + tail), generator=g)]
    flat = x[..., lead:lead + c].reshape(-1)
    flat[:254] = finite[torch.randperm(254, generator=g)]
    x[..., lead:lead + c] = flat.reshape(n, h, w, c)
    assert len(set(x[..., lead:lead + c].reshape(-1).tolist())) == 254 and not e4m3_is_nan(x).any()
    return x, lead, c


@pytest.mark.parametrize('scale', [1, 2])
@pytest.mark.parametrize('layout', ['nhwc', 'nchw_f32'])
def test_f8_copy_channels(device, layout, scale):
    """Channel-slice copy with nearest x2: bytes identical (NHWC), or fp32 byte * dequant with a
    power-of-two dequant, bit for bit (-0 included); everything outside the output slice untouched."""
    x, lead, c = copy_input()
    n, h, w = x.shape[:3]
    src = x[..., lead:lead + c].repeat_interleave(scale, 1).repeat_interleave(scale, 2)
    d = L.CopyDesc()
    d.n, d.h, d.w, d.c, d.in_c_off, d.in_c_stride = n, h, w, c, lead, x.shape[3]
    d.scale, d.dtype = scale, L.DT_FP8
    if layout == 'nhwc':
        d.out_c_off, d.out_c_stride, d.out_layout = OUT_EXTRA, OUT_EXTRA + c + OUT_TAIL, L.OUT_NHWC
        y = torch.full((n, h * scale, w * scale, OUT_EXTRA + c + OUT_TAIL), SENT, dtype=torch.uint8)
        exp = framed(src)
    else:
        d.out_c_off, d.out_c_stride, d.out_layout, d.dequant = 8, c + 16, L.OUT_NCHW_F32, 1 / 32
        y = torch.full((n, c + 16, h * scale, w * scale), SENT_F32)
        exp = y.clone()
        exp[:, 8:8 + c] = (src.view(E4M3).double() / 32).float().permute(0, 3, 1, 2)
    xd, yd = x.to(device), y.to(device)
    L.check(L.lib.ycx_copy_channels(ctypes.byref(d), xd.data_ptr(), yd.data_ptr(), L.stream_handle(device)))
    torch.cuda.synchronize()
    if layout == 'nhwc':
        assert_bytes(yd.cpu(), exp, f"copy scale {scale}")
    else:
        assert_f32_bits(yd.cpu(), exp, f"copy scale {scale} fp32 NCHW")


# ---- SiLU and pre-scaled SiLU at code level ----
# Plain SiLU: z = fma(acc, dq, bias) is exact as above, and the FAST epilogue is within (|z| + 4) 2^-23
# relative of silu(z) (test_gpu_conv_exact.py, above SILU_CASES); the multiply by out_scale is exact.
# YCX_ACT_SILU_PS in fp8 (engine.py packs dq' = fp32(k dq), bias' = fp32(k bias), k = -log2(e); the e4m3
# weights stay): with c = acc dq + bias the true pre-activation and z' = k c, the epilogue's argument is
#   fma(acc, dq', bias') = (acc dq k (1 + d1) + bias k (1 + d2)) (1 + d3),  |d_i| <= 2^-24,
# so it misses z' by at most |k| (|acc dq| + |bias|) 2^-24 + |z'| 2^-24 <= |k| (2 |c| + 2 |bias|) 2^-24
# (|acc dq| <= |c| + |bias|, and |z'| = |k| |c|): the epilogue evaluates silu at c + e, |e| <= (|c| + |bias|) 2^-23.
# That e is ABSOLUTE in c -- acc dq and bias may cancel -- so it moves the result by |silu'(c)| |e| + |e|^2 / 4
# (silu'(c) = s (1 + c (1 - s)), s = sigmoid(c); |silu''| <= 1/2), on top of the evaluation's
# (|z'| + 4) 2^-23 relative. An element is held bit-exact where the
# float64 reference lies farther than twice that total from a rounding boundary of e4m3 (after out_scale), and
# within one code of the expected byte everywhere; the NaN codes are never accepted (helpers.elt_ulps).
SILU_F8_CASES = [(35, 2, 13, 11, 64, 3, 1, 64, 64), (36, 2, 13, 11, 128, 1, 1, 64, 64), (37, 2, 16, 16, 64, 3, 1, 64, 64)]


def silu_f8_operands(n, h, w, cin, k, s, cpad):
    """x in steps of 1/8 of hx = 2^floor(log2(12 / sqrt(K))), w in 1/8 steps within +-1 (z of a few units;
    both e4m3 values), as test_gpu_conv_exact.silu_operands."""
    hx = 2.0 ** math.floor(math.log2(12 / math.sqrt(cin * k * k)))
    return operands(n, h, w, cin, k, s, cpad, seed=3, grid=(hx / 8, 1 / 8, hx, 1.0))


def silu_f8_conditions(c, b, act, what=""):
    """From the exact pre-activation c (NCHW) and the bias alone: the output scale, the float64 reference
    (NHWC, scaled), the excused elements; asserts the input conditions."""
    assert float(c.abs().max()) <= SILU_MAX_Z, "input condition: |c| <= 32"
    cc = c.permute(0, 2, 3, 1).contiguous()
    ref = silu_ref(cc, L.ACT_SILU)
    a = ref.abs().reshape(-1)
    so = next(2.0 ** e for e in range(-16, 17) if float((a * 2.0 ** e > F8_MAX).double().mean()) >= MIN_SAT)
    z = cc * abs(L.SILU_PS_K) if act == L.ACT_SILU_PS else cc
    total = (z.abs() + 4) * 2.0 ** -23 * ref.abs()
    if act == L.ACT_SILU_PS:
        e, sg = (cc.abs() + b.abs().reshape(1, 1, 1, -1)) * 2.0 ** -23, torch.sigmoid(cc)
        total = total + (sg * (1 + cc * (1 - sg))).abs() * e + e * e / 4
    v = ref * so
    lo, hi = elt_neighbours(v.clamp(-F8_MAX, F8_MAX), E4M3)
    excused = (v.abs() <= F8_MAX) & (lo != hi) & ((v - (lo + hi) / 2).abs() <= 2 * total * so)
    share = float(excused.double().mean())
    assert share <= MAX_EXCUSED, f"{what}: input condition, {share:.5f} of the elements are excused"
    return so, v, excused, share


def check_silu_f8(got, v, excused, share, what, lead=OUT_EXTRA, tail=OUT_TAIL):
    """got: the raw buffer; v: the scaled float64 reference NHWC."""
    cout = v.shape[3]
    assert bool((got[..., :lead] == SENT).all() and (got[..., lead + cout:] == SENT).all()), \
        f"{what}: wrote outside the output channel slice"
    g = got[..., lead:lead + cout].contiguous()
    assert not e4m3_is_nan(g).any(), f"{what}: NaN codes stored"
    ulps = elt_ulps(g.view(E4M3), rne(v.clamp(-F8_MAX, F8_MAX), E4M3), E4M3)
    assert int(ulps.abs().max()) <= 1, f"{what}: {int(ulps.abs().max())} codes from the expected byte"
    bad = ~excused & (ulps != 0)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {int((~excused).sum())} elements away from a rounding " \
                          f"boundary differ from the expected byte ({share:.5f} excused)"


@pytest.mark.parametrize('act', [L.ACT_SILU, L.ACT_SILU_PS])
@pytest.mark.parametrize('tile,n,h,w,cin,k,s,cout,cpad', SILU_F8_CASES)
def test_f8_silu_ulps(device, tile, n, h, w, cin, k, s, cout, cpad, act):
    """One case each on tiles 35, 36 and 37. YCX_ACT_SILU_PS: bias and dq rows packed as engine.py does."""
    o = silu_f8_operands(n, h, w, cin, k, s, cpad)
    what = f"tile {tile} act {act}"
    so, v, excused, share = silu_f8_conditions(o.z[:, :cout], o.b[:cout], act, what)
    bias = (o.bias.double() * L.SILU_PS_K).float() if act == L.ACT_SILU_PS else None
    got = launch(device, o, tile, cout, act, 0.0, so, bias=bias)
    check_silu_f8(got, v, excused, share, what)


def stem2_silu_f8_conditions(act):
    """ycx_stem_conv2's SiLU pair computes in bf16 on packed weights: test_gpu_conv_exact's operands (the
    stem map is RNE(silu) whatever the epilogue's last bits; z2 is exact; YCX_ACT_SILU_PS: the packed
    weights themselves are on the grid), margin as there, boundaries those of e4m3 after out_scale."""
    x, ws, bs, wc, bc, z2 = stem2_silu_operands(act, L.DT_BF16)
    assert float(z2.abs().max()) <= SILU_MAX_Z
    zz = z2.permute(0, 2, 3, 1).contiguous()
    ref = silu_ref(zz, act)
    a = ref.abs().reshape(-1)
    so = next(2.0 ** e for e in range(-16, 17) if float((a * 2.0 ** e > F8_MAX).double().mean()) >= MIN_SAT)
    v = ref * so
    lo, hi = elt_neighbours(v.clamp(-F8_MAX, F8_MAX), E4M3)
    margin = (zz.abs() + 8) * 2.0 ** -23 * v.abs()
    excused = (v.abs() <= F8_MAX) & (lo != hi) & ((v - (lo + hi) / 2).abs() <= margin)
    share = float(excused.double().mean())
    assert share <= MAX_EXCUSED, f"stem2 act {act}: input condition, {share:.5f} of the elements are excused"
    return (x, ws, bs, wc, bc), so, v, excused, share


@pytest.mark.parametrize('act', [L.ACT_SILU, L.ACT_SILU_PS])
def test_f8_silu_ulps_stem2(device, act):
    ops, so, v, excused, share = stem2_silu_f8_conditions(act)
    got = run_stem2_f8(device, 1, act, 0.0, so, *ops, 64)
    check_silu_f8(got, v, excused, share, f"stem2 act {act}", 8, 8)
