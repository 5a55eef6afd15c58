"""ycx_classify alone: global average pool over an NHWC channel slice + the dense layer on the fp32 means.

Frame of every case: the input is the channel slice at in_c_off = 8 of a buffer 16 channels wider whose other
channels hold NaN (bf16 / fp16 / f32) or the e4m3 NaN code, so a read outside the slice reaches the logits;
the logits [n][cout] and the workspace [n][c] sit in sentinel frames (helpers.guarded_out / fetch_out) and
are compared whole.

Shapes, the smallest that can go wrong: n in {1, 3}; h x w in {1x1 (the pool is the identity), 5x7 (35 pixels:
odd, fewer rows than waves), 8x8 (exact), 20x20 (several rounds of the pixel loop and a tail)}; c in {8 (one
lane's vector), 72 (one past 64), 520 (one vector past a wave of 64 lanes x 8 channels)}; cout in {1, 10, 65};
every element type. A further case per block shape of the pool (1 .. 64 channel vectors per block) and one for
the 16-byte e4m3 vectors, which a slice at channel 8 never takes.

exact:   integer inputs in [-4, 4], h x w in {1, 4, 16, 64}, weights and bias multiples of 1/4 in [-2, 2]: every
         mean, product and partial sum has at most 21 significant bits, so fp32 holds it exactly in any order
         and logits and workspace must equal the float64 result bit for bit (e4m3: scale 16, a power of two).
bound:   N(0, 1) inputs rounded to the element type; against float64 on those rounded inputs each logit may
         differ by (h w + c + 8) 2^-24 sum_c |w[o,c]| mean_hw |x[n,:,:,c]| + 2^-24 |ref|: the a-priori fp32
         bound of a sum of h w terms, a dot product of c terms, the divide, the bias add and the final
         rounding. Derived, not measured.
repeat:  two launches give the same bits.   NaN: one NaN in image 1 of 3 makes image 1's logits NaN and leaves
         images 0 and 2 bit-equal to the run without it."""
import ctypes
import functools
import itertools

import pytest
import torch

from helpers import E4M3, IN_LEAD, IN_TAIL, SENTINEL_F32, dyadic, fetch_out, guarded_out, nan_frame
from ycx import _lib as L

pytestmark = pytest.mark.gpu

DT = {'bf16': (L.DT_BF16, torch.bfloat16), 'fp16': (L.DT_F16, torch.float16), 'f32': (L.DT_F32, torch.float32),
      'fp8': (L.DT_FP8, E4M3)}
NS, HWS, CS, COUTS = (1, 3), ((1, 1), (5, 7), (8, 8), (20, 20)), (8, 72, 520), (1, 10, 65)
EXACT_HWS = ((1, 1), (2, 2), (2, 8), (8, 8))
F8_SCALE = 16.0  # s_in of the e4m3 cases: stored = e4m3(x * 16), d.dequant = 1 / 16
U = 2.0 ** -24


def elements(x64, name):
    """x64 rounded to the element type -> (the stored tensor, the float64 values it stands for)."""
    tdt = DT[name][1]
    if name == 'fp8':
        q = (x64 * F8_SCALE).clamp(-448, 448).to(torch.float32).to(E4M3)
        return q, q.to(torch.float32).double() / F8_SCALE
    q = x64.to(tdt)
    return q, q.double()


def framed(q, lead=IN_LEAD, tail=IN_TAIL):
    """The stored slice between NaN channels (e4m3: the NaN code 0x7F), as the buffer that goes to the device."""
    if q.dtype != E4M3:
        return nan_frame(q, lead, tail)
    full = torch.full((*q.shape[:-1], lead + q.shape[-1] + tail), 0x7F, dtype=torch.uint8)
    full[..., lead:lead + q.shape[-1]] = q.view(torch.uint8)
    return full


def run(device, name, buf, n, h, w, c, w64, b64, lead=IN_LEAD, launches=1):
    """ycx_classify on the framed buffer (CPU); returns the CPU logits [n][cout] and workspace [n][c], both
    fetched whole from their sentinel frames."""
    cout = w64.shape[0]
    d = L.ClassifyDesc()
    d.n, d.h, d.w, d.c, d.in_c_off, d.in_c_stride = n, h, w, c, lead, buf.shape[-1]
    d.cout, d.dtype, d.dequant = cout, DT[name][0], (1.0 / F8_SCALE if name == 'fp8' else 1.0)
    xd, wd = buf.to(device), w64.to(torch.float32).contiguous().to(device)
    bd = b64.to(torch.float32).to(device) if b64 is not None else None
    outs = []
    for _ in range(launches):
        y = guarded_out(torch.full((n, cout), SENTINEL_F32), device)
        ws = guarded_out(torch.full((n, c), SENTINEL_F32), device)
        L.check(L.lib.ycx_classify(ctypes.byref(d), xd.data_ptr(), wd.data_ptr(), L.ptr(bd), y.data_ptr(),
                                   ws.data_ptr(), L.stream_handle(device)), "ycx_classify")
        torch.cuda.synchronize()
        outs.append((fetch_out(y, SENTINEL_F32, what='logits'), fetch_out(ws, SENTINEL_F32, what='workspace')))
    return outs[0] if launches == 1 else outs


def reference(xr64, w64, b64):
    """float64 (means [n][c], logits [n][cout], the bound's sum_c |w| mean|x| [n][cout])."""
    mean = xr64.sum((1, 2)) / (xr64.shape[1] * xr64.shape[2])
    ref = mean @ w64.t() + (b64 if b64 is not None else 0.0)
    mag = xr64.abs().sum((1, 2)) / (xr64.shape[1] * xr64.shape[2]) @ w64.abs().t()
    return mean, ref, mag


def assert_bound(y, ws, xr64, w64, b64, what):
    n, h, w, c = xr64.shape
    mean, ref, mag = reference(xr64, w64, b64)
    assert not bool(y.isnan().any()) and not bool(ws.isnan().any()), f"{what}: a read outside the slice"
    bound = (h * w + c + 8) * U * mag + U * ref.abs()
    err = (y.double() - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    assert bool((err <= bound).all()), f"{what}: error / bound up to {worst:.3f}"
    # the means: a sum of h w terms and the divide
    mb = (h * w + 2) * U * xr64.abs().sum((1, 2)) / (h * w)
    assert bool(((ws.double() - mean).abs() <= mb).all()), f"{what}: workspace means"
    return worst


@functools.lru_cache(maxsize=None)
def normal_case(n, h, w, c, cout):
    g = torch.Generator().manual_seed(7 + 1000 * n + 100 * h + 10 * w + c + cout)
    return (torch.randn(n, h, w, c, generator=g, dtype=torch.float64),
            torch.randn(cout, c, generator=g, dtype=torch.float64) / c ** 0.5,
            0.1 * torch.randn(cout, generator=g, dtype=torch.float64))


@pytest.mark.parametrize('name', list(DT))
def test_bound_at_every_shape(device, name):
    worst = 0.0
    for n, (h, w), c, cout in itertools.product(NS, HWS, CS, COUTS):
        x64, w64, b64 = normal_case(n, h, w, c, cout)
        q, xr = elements(x64, name)
        y, ws = run(device, name, framed(q), n, h, w, c, w64.float().double(), b64.float().double())
        worst = max(worst, assert_bound(y, ws, xr, w64.float().double(), b64.float().double(),
                                        f"{name} n{n} {h}x{w} c{c} cout{cout}"))
    print(f"\n{name}: largest error / bound over {len(NS) * len(HWS) * len(CS) * len(COUTS)} shapes {worst:.3f}")


@pytest.mark.parametrize('name', list(DT))
def test_exact_on_dyadic_operands(device, name):
    for n, (h, w), c, cout in itertools.product(NS, EXACT_HWS, CS, COUTS):
        g = torch.Generator().manual_seed(11 + 1000 * n + 100 * h + 10 * w + c + cout)
        x64 = dyadic((n, h, w, c), -4, 4, 1, g)
        w64, b64 = dyadic((cout, c), -2, 2, 0.25, g), dyadic((cout,), -2, 2, 0.25, g)
        q, xr = elements(x64, name)
        assert torch.equal(xr, x64)  # the element type holds the operands
        mean, ref, _ = reference(xr, w64, b64)
        assert torch.equal(ref.float().double(), ref) and torch.equal(mean.float().double(), mean)
        y, ws = run(device, name, framed(q), n, h, w, c, w64, b64)
        what = f"{name} n{n} {h}x{w} c{c} cout{cout}"
        assert torch.equal(y.view(torch.int32), ref.float().view(torch.int32)), f"{what}: logits"
        assert torch.equal(ws.view(torch.int32), mean.float().view(torch.int32)), f"{what}: workspace"


def test_null_bias_is_zero(device):
    x64, w64, _ = normal_case(3, 5, 7, 72, 10)
    q, xr = elements(x64, 'bf16')
    y, ws = run(device, 'bf16', framed(q), 3, 5, 7, 72, w64.float().double(), None)
    assert_bound(y, ws, xr, w64.float().double(), None, "bf16 without a bias")


@pytest.mark.parametrize('name', list(DT))
def test_two_launches_give_the_same_bits(device, name):
    n, h, w, c, cout = 3, 20, 20, 520, 65
    x64, w64, b64 = normal_case(n, h, w, c, cout)
    q, _ = elements(x64, name)
    (y0, ws0), (y1, ws1) = run(device, name, framed(q), n, h, w, c, w64, b64, launches=2)
    assert torch.equal(y0.view(torch.int32), y1.view(torch.int32))
    assert torch.equal(ws0.view(torch.int32), ws1.view(torch.int32))


@pytest.mark.parametrize('name', list(DT))
def test_a_nan_stays_in_its_image(device, name):
    n, h, w, c, cout = 3, 5, 7, 72, 10
    x64, w64, b64 = normal_case(n, h, w, c, cout)
    q, _ = elements(x64, name)
    clean = framed(q)
    y0, ws0 = run(device, name, clean, n, h, w, c, w64, b64)
    dirty = clean.clone()
    if name == 'fp8':
        dirty[1, 3, 4, IN_LEAD + 37] = 0x7F
    else:
        dirty[1, 3, 4, IN_LEAD + 37] = float('nan')
    y1, ws1 = run(device, name, dirty, n, h, w, c, w64, b64)
    assert bool(y1[1].isnan().all()) and not bool(y0.isnan().any())
    assert bool(ws1[1, 37].isnan()) and int(ws1.isnan().sum()) == 1
    for i in (0, 2):
        assert torch.equal(y0[i].view(torch.int32), y1[i].view(torch.int32))
        assert torch.equal(ws0[i].view(torch.int32), ws1[i].view(torch.int32))


# (n, c) -> channel vectors per block of the bf16 pool: the launcher halves 64 while half a block covers the
# slice and, down to 8, while the launch has fewer than 512 blocks
BLOCK_SHAPES = [(3, 8, 1), (3, 16, 2), (3, 32, 4), (3, 512, 8), (128, 512, 16), (256, 512, 32), (512, 512, 64),
                (512, 520, 64)]


@pytest.mark.parametrize('n, c, cl', BLOCK_SHAPES)
def test_every_block_shape_of_the_pool(device, n, c, cl):
    h, w, cout = 3, 5, 3
    x64, w64, b64 = normal_case(n, h, w, c, cout)
    q, xr = elements(x64, 'bf16')
    y, ws = run(device, 'bf16', framed(q), n, h, w, c, w64.float().double(), b64.float().double())
    assert_bound(y, ws, xr, w64.float().double(), b64.float().double(), f"bf16 n{n} c{c}: {cl} vectors per block")


@pytest.mark.parametrize('c', [16, 80, 528])
def test_e4m3_sixteen_byte_vectors(device, c):
    """A slice on 16-channel bounds (offset 16 of a buffer 32 wider) takes the 16-byte e4m3 loads."""
    n, h, w, cout = 3, 5, 7, 10
    x64, w64, b64 = normal_case(n, h, w, c, cout)
    q, xr = elements(x64, 'fp8')
    y, ws = run(device, 'fp8', framed(q, 16, 16), n, h, w, c, w64.float().double(), b64.float().double(), lead=16)
    assert_bound(y, ws, xr, w64.float().double(), b64.float().double(), f"fp8 c{c} on 16-channel bounds")
