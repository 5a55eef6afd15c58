"""ycx_maxpool, ycx_copy_channels and the two fused k2 s2 pools at the exact-operand bar:
bit patterns against a float64 torch reference on the CPU, the whole output buffer compared so that
the sentinel (3.0) on both sides of every channel slice must survive, and input conditions asserted
from the reference alone (tests/test_move_plan.py builds every case without a GPU).

The library has one definition of a max-pool, torch.nn.MaxPool2d's: -inf padding, floor mode, and NaN
wherever the window holds a NaN (the 16-bit range guard needs every layer to hand
inf / NaN on). The comparison is on bits with two stated exceptions:
  * where the reference is NaN the result must be NaN, any payload;
  * pool inputs hold no -0.0 (torch keeps the first of two equal values, the hardware max orders the
    zeros: the sign of a zero is not something the pools promise). The copy inputs do hold -0.0 and
    NaN payloads: a copy moves bits.

Pool inputs are drawn in the element type (the float64 image is exact): N(0, 4^2) values of both
signs, and at 1/64 each the largest finite magnitude with either sign, the smallest and the largest
subnormal, another subnormal, +inf and -inf. The first and last two rows and columns are negative (a
pad value of 0 instead of -inf, or a dropped floor-mode tail, shows there); on a map no wider (higher)
than four the columns (rows) are left alone, or nothing positive would remain. Windows of k >= 5 reach
past a two-pixel border, so channels 0 and c - 1 of image 0 are negative throughout as well: every
window of theirs has a negative maximum, also at the third level of a cascade.
NaN variants: NaN at 4 % of the elements of the channels with c % 4 == 1, i.e. about 1 % of all
positions, next to clean lanes in every 16-byte vector, and one block of NaN in the first corner of
channel 1 of the last image, as large as the corner window. Spread over all channels, 1 % would put a
NaN into most windows of a k 13 pool (49 .. 143 elements each); kept to a quarter of the channels the
NaN outputs stay between one and half of all outputs whatever the window, as the conditions demand.

fp8 (e4m3fn) pool inputs are drawn from the 253 codes that are neither NaN (0x7F, 0xFF) nor -0.0
(0x80); e4m3fn has no infinities. The fp8 plan's stores saturate and cannot produce a NaN code, so
what the fp8 pools do with one is out of scope here (their max stays fmaxf).

Cases (common layout: n 2, c 40 = five 16-bit or ten fp32 vectors, the input slice at channel 8 of
a buffer 24 wider, the output slice at channel 16 of a buffer 24 wider):
  test_exact_maxpool                maxpool_rows_kernel<bf16 / fp16 / fp32>, maxpool_f8_kernel
  test_exact_maxpool_flat_fallback  maxpool_kernel<T> (n * ho = 65536 > 65535) against the rows kernel one image below
  test_exact_maxpool_cascade        maxpool_cascade_kernel<2>, <2, true>, <1>, levels 2 and 3 (e4m3 at c % 16 != 0
                                    and, test_cascade_rejects_a_plane_past_the_lds, 46 x 46 x 8: refused)
  test_exact_copy                   copy_kernel<T>, x1 / x2, NHWC (raw bits) and fp32 NCHW (exact widening)
  test_pool_rejects                 the status codes that must come back with no device work
  test_fused_pool_propagates_nan    ycx_conv2d in_pool = 1 (tiles 16, 18, auto); ..._pair_pool: ycx_conv2d_pair_pool
With fmaxf in the pools (the library before ycx_pool_max) the 57 NaN cases of this file fail -- a window with
a NaN comes out finite, one of NaN only as -inf -- and the other 74 pass.
"""
import ctypes
import functools
import types

import pytest
import torch
import torch.nn.functional as F

L = pytest.importorskip("ycx._lib")

F8 = torch.float8_e4m3fn
TDT = {L.DT_BF16: torch.bfloat16, L.DT_F16: torch.float16, L.DT_F32: torch.float32, L.DT_FP8: F8}
ITYPE = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32, F8: torch.uint8}
MANT = {torch.bfloat16: 7, torch.float16: 10, torch.float32: 23}
SENTINEL = 3.0  # representable in every element type, e4m3 included
IN_OFF, OUT_OFF, EXTRA = 8, 16, 24
N, C = 2, 40
NAN_DENSITY, NAN_EVERY = 0.04, 4  # 4 % of the channels c % 4 == 1: about 1 % of all positions
DT_ALL = [L.DT_BF16, L.DT_F16, L.DT_F32, L.DT_FP8]
DT_FLOAT = [L.DT_BF16, L.DT_F16, L.DT_F32]
DT16 = [L.DT_BF16, L.DT_F16]
KSP = [(2, 2, 0), (3, 2, 1), (3, 1, 1), (5, 1, 2), (9, 1, 4), (13, 1, 6)]
CASCADE_SHAPES = [(11, 13, 48, 5), (7, 9, 16, 7), (20, 20, 136, 5), (45, 45, 8, 3)]
FLAT = dict(h=64, w=2, c=8, k=2, s=2, p=0)  # n 2048: n * ho = 65536, the grid-stride kernel; n 2047: the rows kernel


def bits(t):
    return t.contiguous().view(ITYPE[t.dtype])


def to_elt(t64, tdt):
    """float64 -> element type; every value here is representable, so the cast is exact."""
    return t64.float().to(F8) if tdt == F8 else t64.to(tdt)


def widen(t):
    return (t.float() if t.dtype == F8 else t).double()


def maps(s):
    return [(11, 13)] + ([(12, 16)] if s == 2 else [])


def _seed(*a):
    v = 7
    for x in a:
        v = (v * 1000003 + int(x)) % (1 << 31)
    return v


def pool_values(tdt, shape, nan, corner, gen):
    """The slice [n][h][w][c] of one pool input as float64 (module docstring). corner: (rows, cols) of
    the first output's window inside the image, the size of the all-NaN block."""
    n, h, w, c = shape
    if tdt == F8:
        codes = torch.tensor([b for b in range(256) if b not in (0x7F, 0xFF, 0x80)], dtype=torch.uint8)
        v = codes[torch.randint(0, len(codes), shape, generator=gen)].view(F8).float().double()
        assert bool(torch.isfinite(v).all()) and float(v.abs().max()) == 448.0
    else:
        fi = torch.finfo(tdt)
        tiny = fi.smallest_normal * fi.eps  # the smallest subnormal
        v = (torch.randn(shape, generator=gen) * 4).to(tdt).double()
        sel = torch.randint(0, 64, shape, generator=gen)
        for i, s in enumerate([fi.max, -fi.max, tiny, fi.smallest_normal - tiny, -3 * tiny, float('inf'),
                               -float('inf')]):
            v[sel == i] = s
    v[v == 0] = 0.0  # no -0.0
    neg = -v.abs()
    neg[neg == 0] = -1.0
    border = torch.zeros(h, w, dtype=torch.bool)
    if h > 4:
        border[:2] = border[-2:] = True
    if w > 4:
        border[:, :2] = border[:, -2:] = True
    v[:, border] = neg[:, border]
    for ch in (0, c - 1):
        v[0, :, :, ch] = neg[0, :, :, ch]
    if nan:
        assert tdt != F8
        m = torch.rand(shape, generator=gen) < NAN_DENSITY
        m[..., [ch for ch in range(c) if ch % NAN_EVERY != 1]] = False
        v[m] = float('nan')
        v[n - 1, :corner[0], :corner[1], 1] = float('nan')
    return v


@functools.lru_cache(maxsize=None)
def pool_case(dtype, n, h, w, c, k, s, p, levels=1, nan=False, in_off=IN_OFF, in_extra=EXTRA):
    """One pool problem, built once and never modified: x (the whole input buffer in the element type,
    SENTINEL around the slice), ref (per level, float64 [n][ho][wo][c]: F.max_pool2d on the float64
    image, level after level) and exp (the whole expected output buffer in the element type)."""
    tdt = TDT[dtype]
    o = types.SimpleNamespace(dtype=dtype, tdt=tdt, n=n, h=h, w=w, c=c, k=k, s=s, p=p, levels=levels, nan=nan,
                              in_off=in_off, in_stride=c + in_extra)
    o.ho, o.wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    o.out_stride = levels * c + EXTRA
    gen = torch.Generator().manual_seed(_seed(dtype, n, h, w, c, k, s, p, levels, nan))
    v = pool_values(tdt, (n, h, w, c), nan, (min(k - p, h), min(k - p, w)), gen)
    x64 = torch.full((n, h, w, o.in_stride), SENTINEL, dtype=torch.float64)
    x64[..., in_off:in_off + c] = v
    o.x = to_elt(x64, tdt)
    back = widen(o.x)
    assert torch.equal(back.isnan(), x64.isnan()) and torch.equal(back.nan_to_num(nan=0.0), x64.nan_to_num(nan=0.0))
    assert not bool(((back == 0) & torch.signbit(back)).any())  # no -0.0 went in
    o.nan_windows = None
    cur, o.ref = v.permute(0, 3, 1, 2), []
    if nan:  # 1 where the whole first-level window is NaN: a min-pool of the NaN mask (padding never wins)
        o.nan_windows = -F.max_pool2d(-cur.isnan().double(), k, s, p)
    for _ in range(levels):
        cur = F.max_pool2d(cur, k, s, p)
        o.ref.append(cur.permute(0, 2, 3, 1).contiguous())
    e64 = torch.full((n, o.ho, o.wo, o.out_stride), SENTINEL, dtype=torch.float64)
    for lv, r in enumerate(o.ref):
        e64[..., OUT_OFF + lv * c:OUT_OFF + (lv + 1) * c] = r
    o.exp = to_elt(e64, tdt)
    assert torch.equal(widen(o.exp).nan_to_num(nan=0.0), e64.nan_to_num(nan=0.0))  # a max is one of the inputs
    return o


def check_pool_conditions(o, what=""):
    """The input conditions of a pool case, from the float64 reference alone."""
    edge = torch.zeros(o.ho, o.wo, dtype=torch.bool)
    edge[0] = edge[-1] = True
    edge[:, 0] = edge[:, -1] = True
    for lv, r in enumerate(o.ref):
        b = r[:, edge]
        assert bool((torch.isfinite(b) & (b < 0)).any()), f"{what} level {lv}: no border window with a negative maximum"
        if o.tdt != F8:
            assert bool((r == float('inf')).any()), f"{what} level {lv}: no inf among the outputs"
        share = float(r.isnan().double().mean())
        if o.nan:
            assert 1 <= int(r.isnan().sum()) and share <= 0.5, f"{what} level {lv}: {share:.3f} of the outputs are NaN"
        else:
            assert share == 0.0
    if o.nan:
        assert bool((o.nan_windows == 1).any()), f"{what}: no window of NaN only"
    return o


def pool_desc(o):
    d = L.PoolDesc()
    d.n, d.h, d.w, d.c, d.in_c_off, d.in_c_stride = o.n, o.h, o.w, o.c, o.in_off, o.in_stride
    d.ho, d.wo, d.out_c_off, d.out_c_stride = o.ho, o.wo, OUT_OFF, o.out_stride
    d.k, d.stride, d.pad, d.dtype, d.levels = o.k, o.s, o.p, o.dtype, o.levels
    return d


def sentinel_like(shape, tdt, device):
    return bits(to_elt(torch.full(shape, SENTINEL, dtype=torch.float64), tdt)).to(device)


def run_pool(device, o):
    """One ycx_maxpool through the C ABI; the raw output buffer (SENTINEL-filled before the launch)."""
    xd, yd = bits(o.x).to(device), sentinel_like((o.n, o.ho, o.wo, o.out_stride), o.tdt, device)
    L.check(L.lib.ycx_maxpool(ctypes.byref(pool_desc(o)), xd.data_ptr(), yd.data_ptr(), L.stream_handle(device)),
            "ycx_maxpool")
    torch.cuda.synchronize()
    return yd.cpu().view(o.tdt)


def assert_same(got, exp, what=""):
    """Bit patterns of two element-type tensors; where exp is NaN, got must be NaN (any payload)."""
    assert got.shape == exp.shape and got.dtype == exp.dtype, (got.shape, exp.shape, got.dtype, exp.dtype)
    if got.dtype == F8:  # the e4m3 cases hold no NaN: bytes
        bad = bits(got) != bits(exp)
    else:
        bad = torch.where(exp.isnan(), ~got.isnan(), bits(got) != bits(exp))
    if bool(bad.any()):
        at = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the reference (or the "
                             f"sentinel); first at {at}: got {float(widen(got)[at])!r}, want {float(widen(exp)[at])!r}")


def nans(dtype):
    return (False,) if dtype == L.DT_FP8 else (False, True)


def with_nans(dtypes):
    """(dtype, nan) parameters: every type clean, the float types also with NaN."""
    return [pytest.param(dt, nan, id=f"dt{dt}-{'nan' if nan else 'clean'}") for dt in dtypes for nan in nans(dt)]


@pytest.mark.gpu
@pytest.mark.parametrize('dtype,nan', with_nans(DT_ALL))
@pytest.mark.parametrize('k,s,p', KSP)
def test_exact_maxpool(device, k, s, p, dtype, nan):
    """Every (k, s, p) the networks use plus k3 s2 p1 and k3 s1, 11 x 13 (stride 2 also 12 x 16), with and
    without NaN: the window clamped at every border, the floor-mode tail, 40 channels, both slices."""
    for h, w in maps(s):
        what = f"k{k} s{s} p{p} {h}x{w} dtype {dtype} nan {nan}"
        o = check_pool_conditions(pool_case(dtype, N, h, w, C, k, s, p, 1, nan), what)
        assert_same(run_pool(device, o), o.exp, what)


def flat_side(o):
    """ycx_maxpool's dispatch, from the descriptor: True when the grid-stride kernel runs."""
    vn = 4 if o.dtype == L.DT_F32 else 8
    rows, total = o.n * o.ho, o.n * o.ho * o.wo * (o.c // vn)
    return o.dtype == L.DT_FP8 or rows > 65535 or total >= 1 << 31 or o.n * o.h * o.w * o.in_stride >= 1 << 31


def flat_case(dtype, n, nan):
    f = FLAT
    return pool_case(dtype, n, f['h'], f['w'], f['c'], f['k'], f['s'], f['p'], 1, nan, in_off=0, in_extra=0)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DT_FLOAT)
@pytest.mark.parametrize('n,nan', [(2048, False), (2047, False), (2048, True)])
def test_exact_maxpool_flat_fallback(device, n, nan, dtype):
    """k2 s2 on n x 64 x 2 x 8 (a dense 4 MB input in 16-bit): n 2048 gives n * ho = 65536 output rows, one
    more than a grid's y extent, so the grid-stride kernel with its 64-bit index chain runs; n 2047 stays
    with the rows kernel. Both against the one reference; the NaN variant on the grid-stride side."""
    o = check_pool_conditions(flat_case(dtype, n, nan), f"flat n {n} dtype {dtype}")
    assert o.n * o.ho == (65536 if n == 2048 else 65504) and flat_side(o) == (n == 2048)
    assert_same(run_pool(device, o), o.exp, f"flat n {n} dtype {dtype} nan {nan}")


def cascade_case(dtype, h, w, c, k, levels, nan):
    return pool_case(dtype, N, h, w, c, k, 1, k // 2, levels, nan)


def cascade_slice(o):
    """ycx_maxpool's channel slice per workgroup: the widest power of two that divides c whose two planes fit 64 KB."""
    esz = 1 if o.dtype == L.DT_FP8 else 2
    return next((t for t in (128, 64, 32, 16, 8) if t * esz >= 16 and o.c % t == 0 and 2 * o.h * o.w * t * esz <= 65536), 0)


def assert_pool_refused(device, o, status, what=""):
    """ycx_maxpool returns ``status`` for o's descriptor and writes nothing."""
    tdt = TDT[o.dtype]
    xd = sentinel_like((o.n, o.h, o.w, o.in_stride), tdt, device)
    yd = sentinel_like((o.n, o.ho, o.wo, o.out_stride), tdt, device)
    got = L.lib.ycx_maxpool(ctypes.byref(pool_desc(o)), xd.data_ptr(), yd.data_ptr(), L.stream_handle(device))
    torch.cuda.synchronize()
    assert got == status, f"{what}: status {got}"
    assert torch.equal(yd.cpu(), sentinel_like(yd.shape, tdt, 'cpu')), what


def cascade_shell(dtype, h, w, c, k, levels):
    """The descriptor fields of a cascade without its data."""
    return types.SimpleNamespace(dtype=dtype, n=N, h=h, w=w, c=c, k=k, s=1, p=k // 2, levels=levels, in_off=IN_OFF,
                                 in_stride=c + EXTRA, ho=h, wo=w, out_stride=levels * c + EXTRA)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype,nan', with_nans([L.DT_BF16, L.DT_F16, L.DT_FP8]))
@pytest.mark.parametrize('levels', [2, 3])
@pytest.mark.parametrize('h,w,c,k', CASCADE_SHAPES)
def test_exact_maxpool_cascade(device, h, w, c, k, levels, dtype, nan):
    """levels 'same' pools in one launch, level i at out_c_off + i * c, vs F.max_pool2d level after level:
    an odd map, one smaller than a window of the third level, 17 slices per image (c 136), and the
    largest 16-bit plane that fits the LDS (45 x 45 x 8). The e4m3 cascade moves 16-byte chunks of 16
    channels: at c 136 and c 8 no slice divides c and the call must be refused (UNSUPPORTED, nothing
    written) -- the engine then runs the levels as single pools."""
    if (h, w, c) == (45, 45, 8):
        assert 2 * h * w * 8 * 2 <= 65536 < 2 * 46 * 46 * 8 * 2
    if dtype == L.DT_FP8 and c % 16:
        shell = cascade_shell(dtype, h, w, c, k, levels)
        assert cascade_slice(shell) == 0
        return assert_pool_refused(device, shell, L.YCX_ERR_UNSUPPORTED, f"fp8 cascade c{c}")
    what = f"cascade {h}x{w} c{c} k{k} levels {levels} dtype {dtype} nan {nan}"
    o = check_pool_conditions(cascade_case(dtype, h, w, c, k, levels, nan), what)
    assert cascade_slice(o) > 0
    assert_same(run_pool(device, o), o.exp, what)


@pytest.mark.gpu
def test_cascade_rejects_a_plane_past_the_lds(device):
    """46 x 46 x 8 in bf16: two planes of the narrowest slice are 67712 bytes: UNSUPPORTED, nothing written."""
    shell = cascade_shell(L.DT_BF16, 46, 46, 8, 3, 3)
    assert cascade_slice(shell) == 0
    assert_pool_refused(device, shell, L.YCX_ERR_UNSUPPORTED, "46 x 46 x 8")


# ---- copy / nearest x2 ----
COPY_SHAPE = (2, 5, 7, 24)


def special_bits(tdt):
    """-0.0, the infinities, four NaNs (quiet, quiet with a payload, signalling, negative), the
    smallest and largest subnormal and the largest finite value, as bit patterns of the element type."""
    m, width = MANT[tdt], 16 if ITYPE[tdt] == torch.int16 else 32
    sign, inf = 1 << (width - 1), ((1 << (width - 1 - m)) - 1) << m
    qnan = inf | 1 << (m - 1)
    vals = [sign, inf, sign | inf, qnan, qnan | 5, inf | 1, sign | qnan | 1, 1, (1 << m) - 1, inf - 1]
    return [v - (1 << width) if v & sign else v for v in vals]  # as the signed integer type holds them


@functools.lru_cache(maxsize=None)
def copy_input(dtype):
    """x: the input buffer of the copy cases (SENTINEL around the slice at channel 8); every special
    pattern of special_bits at six places of the slice. Never modified."""
    tdt, (n, h, w, c) = TDT[dtype], COPY_SHAPE
    gen = torch.Generator().manual_seed(_seed(dtype, 77))
    b = bits((torch.randn(n, h, w, c, generator=gen) * 4).to(tdt)).clone().view(-1)
    sp = special_bits(tdt)
    where = torch.randperm(b.numel(), generator=gen)[:6 * len(sp)]
    b[where] = torch.tensor(sp, dtype=b.dtype).repeat(6)
    x = to_elt(torch.full((n, h, w, c + EXTRA), SENTINEL, dtype=torch.float64), tdt)
    xb = bits(x)
    xb[..., IN_OFF:IN_OFF + c] = b.view(n, h, w, c)
    x = xb.view(tdt)
    sl = x[..., IN_OFF:IN_OFF + c]
    assert len(set(bits(sl[sl.isnan()]).tolist())) == 4 and bool(((sl == 0) & torch.signbit(sl)).any())
    assert bool(sl.isinf().any()) and set(sp) <= set(bits(sl).view(-1).tolist())
    return x


def copy_expected(dtype, scale, nchw):
    """F.interpolate(mode='nearest') on the float64 image: of the bit patterns for the NHWC copy (a copy
    moves bits; every 16- and 32-bit integer is a float64), of the values for the widening fp32 NCHW store."""
    tdt, (n, h, w, c) = TDT[dtype], COPY_SHAPE
    sl = copy_input(dtype)[..., IN_OFF:IN_OFF + c]
    if nchw:
        exp = torch.full((n, c + 16, h * scale, w * scale), SENTINEL, dtype=torch.float32)
        up = F.interpolate(sl.double().permute(0, 3, 1, 2), scale_factor=scale, mode='nearest')
        exp[:, 8:8 + c] = up.float()  # exact: fp32 holds every 16-bit value
        assert torch.equal(exp.double().nan_to_num(nan=0.0)[:, 8:8 + c], up.nan_to_num(nan=0.0))
        return exp
    up = F.interpolate(bits(sl).double().permute(0, 3, 1, 2), scale_factor=scale, mode='nearest').permute(0, 2, 3, 1)
    exp = bits(to_elt(torch.full((n, h * scale, w * scale, c + EXTRA), SENTINEL, dtype=torch.float64), tdt))
    exp[..., OUT_OFF:OUT_OFF + c] = up.to(exp.dtype)
    return exp


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DT_FLOAT)
@pytest.mark.parametrize('scale', [1, 2])
@pytest.mark.parametrize('nchw', [False, True])
def test_exact_copy(device, nchw, scale, dtype):
    """NHWC: raw bits, NaN payloads and -0.0 included, x1 and the nearest x2. fp32 NCHW (at plane 8 of
    c + 16 planes): the exact widening with -0.0 kept, NaN where the input is NaN; the sentinel planes intact."""
    tdt, (n, h, w, c) = TDT[dtype], COPY_SHAPE
    exp = copy_expected(dtype, scale, nchw)
    d = L.CopyDesc()
    d.n, d.h, d.w, d.c, d.in_c_off, d.in_c_stride, d.scale, d.dtype = n, h, w, c, IN_OFF, c + EXTRA, scale, dtype
    if nchw:
        d.out_c_off, d.out_c_stride, d.out_layout = 8, c + 16, L.OUT_NCHW_F32
        yd = torch.full(exp.shape, SENTINEL, dtype=torch.float32, device=device)
    else:
        d.out_c_off, d.out_c_stride, d.out_layout = OUT_OFF, c + EXTRA, L.OUT_NHWC
        yd = sentinel_like(exp.shape, tdt, device)
    xd = bits(copy_input(dtype)).to(device)
    L.check(L.lib.ycx_copy_channels(ctypes.byref(d), xd.data_ptr(), yd.data_ptr(), L.stream_handle(device)),
            "ycx_copy_channels")
    torch.cuda.synchronize()
    what = f"copy dtype {dtype} x{scale} {'nchw_f32' if nchw else 'nhwc'}"
    if nchw:
        assert_same(yd.cpu(), exp, what)
    else:
        got = yd.cpu()
        assert got.dtype == exp.dtype and got.shape == exp.shape
        bad = got != exp
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements are not the input's bits; first at " \
                                    f"{[int(v) for v in bad.nonzero()[0]] if bool(bad.any()) else None}"


# ---- rejected descriptors ----
def _small_pool():
    d = L.PoolDesc()
    d.n, d.h, d.w, d.c, d.in_c_off, d.in_c_stride = 1, 8, 8, 16, 8, 32
    d.ho, d.wo, d.out_c_off, d.out_c_stride, d.k, d.stride, d.pad, d.dtype, d.levels = 8, 8, 16, 64, 3, 1, 1, L.DT_BF16, 1
    return d


def _small_copy():
    d = L.CopyDesc()
    d.n, d.h, d.w, d.c, d.in_c_off, d.in_c_stride = 1, 4, 4, 16, 8, 32
    d.out_c_off, d.out_c_stride, d.scale, d.dtype, d.out_layout = 16, 64, 1, L.DT_BF16, L.OUT_NHWC
    return d


def _edit(d, **kw):
    for k, v in kw.items():
        setattr(d, k, v)
    return d


REJECTS = [
    ('pool', 'pad * 2 > k', dict(k=3, pad=2, ho=10, wo=10), L.YCX_ERR_BAD_ARG),
    ('pool', 'wrong ho', dict(ho=7), L.YCX_ERR_BAD_ARG),
    ('pool', 'c 12 in bf16', dict(c=12), L.YCX_ERR_UNSUPPORTED),
    ('pool', 'levels 3 at stride 2', dict(levels=3, stride=2, ho=4, wo=4), L.YCX_ERR_BAD_ARG),
    ('pool', 'levels 3 in fp32', dict(levels=3, dtype=L.DT_F32), L.YCX_ERR_UNSUPPORTED),
    ('copy', 'scale 3', dict(scale=3), L.YCX_ERR_BAD_ARG),
    ('copy', 'slice past its stride', dict(out_c_off=56), L.YCX_ERR_BAD_ARG),
]


@pytest.mark.gpu
@pytest.mark.parametrize('op,what,edit,status', REJECTS, ids=[r[1].replace(' ', '_') for r in REJECTS])
def test_pool_rejects(device, op, what, edit, status):
    """The status comes back and nothing ran: the output (sized for the valid descriptor, with room to
    spare, 4-byte elements) still holds the sentinel everywhere."""
    d = _edit(_small_pool() if op == 'pool' else _small_copy(), **edit)
    xd = torch.full((16 * 16 * 64,), SENTINEL, dtype=torch.float32, device=device)
    yd = torch.full((16 * 16 * 64,), SENTINEL, dtype=torch.float32, device=device)
    fn = L.lib.ycx_maxpool if op == 'pool' else L.lib.ycx_copy_channels
    got = fn(ctypes.byref(d), xd.data_ptr(), yd.data_ptr(), L.stream_handle(device))
    torch.cuda.synchronize()
    assert got == status, f"{what}: status {got}"
    assert bool((yd == SENTINEL).all()) and bool((xd == SENTINEL).all()), what
    valid = _small_pool() if op == 'pool' else _small_copy()  # the unedited descriptor is accepted
    assert fn(ctypes.byref(valid), xd.data_ptr(), yd.data_ptr(), L.stream_handle(device)) == L.YCX_OK
    torch.cuda.synchronize()


# ---- the fused pools: one NaN in, NaN at its pooled pixel, everything else as the clean launch ----
PIXEL_TILE = 128  # pixels per block of tiles 16 and 18 (launch_glds<BM, 128, ...>)
F1_SHAPES = [(2, 13, 11, 64, 128), (1, 5, 7, 128, 256)]  # n, pooled h x w, cin, cout


def f1_nan_site(n, h, w):
    """(image, pooled row, pooled column) of the last pooled pixel but one: in the ragged last pixel tile."""
    m = n * h * w
    p = m - 2
    assert m % PIXEL_TILE and p >= m // PIXEL_TILE * PIXEL_TILE
    return p // (h * w), p % (h * w) // w, p % w


def assert_only_nan_at(got, clean, site, c0, c1, what):
    """got[site][c0:c1] is NaN in every channel; every other element of the buffer has clean's bits."""
    assert not bool(clean.isnan().any()), f"{what}: the clean launch holds NaN"
    hit = got[site][c0:c1]
    assert bool(hit.isnan().all()), f"{what}: {int((~hit.isnan()).sum())} of {hit.numel()} channels at {site} are not NaN"
    mask = torch.zeros(got.shape, dtype=torch.bool)
    mask[site][c0:c1] = True
    bad = (bits(got) != bits(clean)) & ~mask
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements away from {site} differ from the clean launch; " \
                                f"first at {[int(v) for v in bad.nonzero()[0]] if bool(bad.any()) else None}"


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DT16)
@pytest.mark.parametrize('tile', [16, 18, 0])
@pytest.mark.parametrize('n,h,w,cin,cout', F1_SHAPES)
def test_fused_pool_propagates_nan(device, n, h, w, cin, cout, tile, dtype):
    """ycx_conv2d with in_pool = 1 on test_gpu_conv_exact's operands (leaky 0.125, exact): the clean launch is
    RNE(true sum); with one NaN in x, in the second row of the window of a pooled pixel of the ragged last
    tile, that pixel is NaN in every output channel and nothing else moves."""
    import test_gpu_conv_exact as E
    o = E.operands(dtype, n, h, w, cin, 1, 1, pool=True, cout=cout)
    tdt, (act, slope) = TDT[dtype], E.ACTS[1]
    what = f"in_pool tile {tile} {h}x{w} cin {cin} dtype {dtype}"
    clean = E.launch(device, o, tile, cout, act, slope)
    E.assert_bits(clean, E.expected(E.apply_act(o.z[:, :cout], act, slope), tdt), what)
    img, py, px = f1_nan_site(n, h, w)
    x = o.x_full.clone()
    x[img, 2 * py + 1, 2 * px, o.in_extra + cin - 3] = float('nan')
    got = E.launch(device, types.SimpleNamespace(**{**vars(o), 'x_full': x}), tile, cout, act, slope)
    assert_only_nan_at(got, clean, (img, py, px), 16, 16 + cout, what)


F2_CASES = [((2, 4, 32), 64, 128, 128, (L.ACT_LEAKY, L.ACT_SILU_PS, L.ACT_NONE)),
            ((1, 6, 64), 256, 248, 120, (L.ACT_SILU_PS, L.ACT_LEAKY, L.ACT_LEAKY))]


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DT16)
@pytest.mark.parametrize('store_a', [True, False])
@pytest.mark.parametrize('shape,cin,cout_b,cout_c,acts', F2_CASES)
def test_fused_pool_propagates_nan_pair_pool(device, shape, cin, cout_b, cout_c, acts, store_a, dtype):
    """ycx_conv2d_pair_pool, ya stored and null: a NaN at one pixel of x (odd row, odd column) makes ya and
    yb NaN at that pixel and yc NaN at its pooled pixel, in all channels; everything else, the sentinel
    around the three slices included, is bit-identical to the clean launch."""
    from trio_case import X_OFF, YA_OFF, YB_OFF, YC_OFF, TrioCase
    case = TrioCase(device, dtype, shape, cin, cout_b, cout_c, acts)
    n, h, w = shape
    img, yy, xx = n - 1, h - 1, w - 3

    def run():
        outs = [torch.full_like(t, SENTINEL) for t in case.outputs()]
        L.check(case.fused_status(*outs, store_a), "ycx_conv2d_pair_pool")
        torch.cuda.synchronize()
        return [t.cpu() for t in outs]

    clean = run()
    x = case.host['x'].clone()
    x[img, yy, xx, X_OFF + 5] = float('nan')
    case.dev['x'] = x.to(device)
    ya, yb, yc = run()
    what = f"pair_pool {shape} cin {cin} dtype {dtype} ya {'stored' if store_a else 'null'}"
    if store_a:
        assert_only_nan_at(ya, clean[0], (img, yy, xx), YA_OFF, YA_OFF + 256, what + " ya")
    else:
        assert bool((ya == SENTINEL).all()) and bool((clean[0] == SENTINEL).all()), what + ": ya written"
    assert_only_nan_at(yb, clean[1], (img, yy, xx), YB_OFF, YB_OFF + cout_b, what + " yb")
    assert_only_nan_at(yc, clean[2], (img, yy // 2, xx // 2), YC_OFF, YC_OFF + cout_c, what + " yc")
