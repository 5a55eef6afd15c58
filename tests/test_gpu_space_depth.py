"""ycx_space_depth called directly, bit for bit: the whole output buffer, on its integer view, against the
index formulas of include/ycx.h written out in numpy,

  Contract  y[n, ho, wo, (a*s+b)*C + c]  = x[n, ho*s+a, wo*s+b, c]
  Expand    y[n, h*s+a, w*s+b, c']       = x[n, h, w, (a*s+b)*C' + c'],  C' = C / (s*s)
  Focus     y[n, ho, wo, (2*b+a)*C + c]  = x[n, 2*ho+a, 2*wo+b, c]

as one strided slice assignment per pixel phase (a, b). Input and output are channel slices in the middle
of wider buffers; the output buffer is pre-filled with the sentinel (the bits of 3.0), which must survive
on both sides of the slice. The inputs are uniform random BITS of the element's width, so every class of
value occurs; planted on top: quiet and signalling NaN payloads of both signs, -0.0, +-inf, the smallest
and largest subnormals (16- and 32-bit), and all 256 e4m3 codes (fp8). A move may change none of them.

Shapes (n, h, w, C): (2, 6, 10, 8) and (2, 6, 10, 24) for Contract and Focus at gain 2; (1, 9, 6, 8) and
(1, 9, 6, 24) for Contract at gain 3 (a non-power-of-two gain and a run of three vectors: shift-and-mask
indexing fails there); (2, 3, 5, 32) and (1, 2, 3, 72) for Expand at gains 2 and 3; gain 4 each way. Every
case has more than one 256-lane block or a ragged last one. LAYOUTS[0] puts the slices on 8-channel bounds
(the 8-byte vectors of an e4m3 move), LAYOUTS[1] on 16-channel bounds with runs of 16 (its 16-byte vectors).
The large case moves 2^22 fp32 elements = 2^20 vectors: the launch is capped at 2048 blocks of 256 lanes,
so every lane runs the grid-stride loop twice. (A flat index past 2^32 vectors, where the kernel
decomposes it in 64 bits instead of 32, would need two 64 GiB buffers and is not run here.)"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from test_depth_plan import bad_descs, sdesc, unsupported_descs

L = pytest.importorskip("ycx._lib")

pytestmark = pytest.mark.gpu

ITYPE = {L.DT_BF16: np.uint16, L.DT_F16: np.uint16, L.DT_F32: np.uint32, L.DT_FP8: np.uint8}
SENTINEL = {L.DT_BF16: 0x4040, L.DT_F16: 0x4200, L.DT_F32: 0x40400000, L.DT_FP8: 0x44}  # 3.0
# NaN payloads (quiet, signalling, both signs), -0.0, +-inf, smallest / largest subnormal, all ones
PLANTED = {
    L.DT_BF16: [0x7FC0, 0x7FC1, 0x7F81, 0xFFC0, 0xFFFF, 0xFF85, 0x8000, 0x7F80, 0xFF80, 0x0001, 0x007F, 0x8001],
    L.DT_F16: [0x7E00, 0x7E01, 0x7C01, 0xFE00, 0xFFFF, 0xFC05, 0x8000, 0x7C00, 0xFC00, 0x0001, 0x03FF, 0x8001],
    L.DT_F32: [0x7FC00000, 0x7FC00001, 0x7F800001, 0xFFC00000, 0xFFFFFFFF, 0xFF800005, 0x80000000, 0x7F800000,
               0xFF800000, 0x00000001, 0x007FFFFF, 0x80000001],
    L.DT_FP8: list(range(256)),
}
DT_ALL = [L.DT_BF16, L.DT_F16, L.DT_F32, L.DT_FP8]
LAYOUTS = [(8, 24, 16, 24), (16, 32, 32, 48)]  # in_c_off, input channels beside the slice, out_c_off, output ...
C, E, F = L.SD_CONTRACT, L.SD_EXPAND, L.SD_FOCUS
CASES = [  # mode, gain, (n, h, w, C), layout
    (C, 2, (2, 6, 10, 8), 0), (C, 2, (2, 6, 10, 24), 0), (F, 2, (2, 6, 10, 8), 0), (F, 2, (2, 6, 10, 24), 0),
    (C, 3, (1, 9, 6, 8), 0), (C, 3, (1, 9, 6, 24), 0),
    (E, 2, (2, 3, 5, 32), 0), (E, 3, (1, 2, 3, 72), 0), (E, 3, (1, 2, 3, 216), 0),
    (C, 4, (1, 8, 4, 8), 0), (E, 4, (1, 2, 3, 128), 0),
    (C, 2, (2, 6, 10, 16), 1), (F, 2, (2, 6, 10, 48), 1), (E, 2, (2, 3, 5, 64), 1), (C, 3, (1, 9, 6, 16), 1),
    (E, 4, (1, 2, 3, 256), 1),
]
BIG = (C, 2, (4, 128, 128, 64), 0)  # 2^22 elements
IDS = {C: 'contract', E: 'expand', F: 'focus'}


def out_shape(mode, s, shape):
    n, h, w, c = shape
    return (n, h * s, w * s, c // (s * s)) if mode == E else (n, h // s, w // s, c * s * s)


def move(mode, s, x):
    """The header's index formulas on an [n][h][w][c] array."""
    n, h, w, c = x.shape
    y = np.empty(out_shape(mode, s, x.shape), x.dtype)
    for a in range(s):
        for b in range(s):
            if mode == E:
                r = c // (s * s)
                y[:, a::s, b::s, :] = x[:, :, :, (a * s + b) * r:(a * s + b + 1) * r]
            else:
                q = 2 * b + a if mode == F else a * s + b
                y[:, :, :, q * c:(q + 1) * c] = x[:, a::s, b::s, :]
    return y


@functools.lru_cache(maxsize=None)
def case(dtype, mode, s, shape, layout):
    """One problem, built once and never modified: the whole input buffer (random bits, the planted patterns
    inside the slice), the descriptor fields and the whole expected output buffer."""
    it = ITYPE[dtype]
    n, h, w, c = shape
    in_off, in_extra, out_off, out_extra = LAYOUTS[layout]
    rng = np.random.default_rng([dtype, mode, s, *shape, layout])
    xb = rng.integers(0, np.iinfo(it).max, size=(n, h, w, c + in_extra), dtype=it, endpoint=True)
    x = xb[..., in_off:in_off + c]
    planted = np.array(PLANTED[dtype], it)
    flat = rng.permutation(x.size)[:len(planted)]
    idx = np.unravel_index(flat, x.shape)
    x[idx] = planted  # x is a view: this lands in xb
    assert set(planted.tolist()) <= set(x.reshape(-1).tolist())
    on, oh, ow, oc = out_shape(mode, s, shape)
    exp = np.full((on, oh, ow, oc + out_extra), SENTINEL[dtype], it)
    exp[..., out_off:out_off + oc] = move(mode, s, x)
    return xb, exp


def desc(dtype, mode, s, shape, layout):
    n, h, w, c = shape
    in_off, in_extra, out_off, out_extra = LAYOUTS[layout]
    _, oh, ow, oc = out_shape(mode, s, shape)
    d = L.DepthDesc()
    d.n, d.h, d.w, d.c, d.in_c_off, d.in_c_stride = n, h, w, c, in_off, c + in_extra
    d.ho, d.wo, d.out_c_off, d.out_c_stride = oh, ow, out_off, oc + out_extra
    d.gain, d.mode, d.dtype = s, mode, dtype
    return d


def run(device, d, xb, out_like, dtype):
    x = torch.from_numpy(xb.view(np.uint8)).to(device)
    y = torch.from_numpy(np.full(out_like.shape, SENTINEL[dtype], out_like.dtype).view(np.uint8)).to(device)
    st = L.lib.ycx_space_depth(ctypes.byref(d), x.data_ptr(), y.data_ptr(), L.stream_handle(device))
    assert st == L.YCX_OK, st
    torch.cuda.synchronize()
    return y.cpu().numpy().view(out_like.dtype).reshape(out_like.shape)


def check(got, exp, what):
    bad = np.argwhere(got != exp)
    assert len(bad) == 0, f"{what}: {len(bad)} of {exp.size} elements differ, first at {bad[0].tolist()}: " \
                          f"{got[tuple(bad[0])]:#x} != {exp[tuple(bad[0])]:#x}"


@pytest.mark.parametrize('dtype', DT_ALL, ids=['bf16', 'fp16', 'f32', 'fp8'])
@pytest.mark.parametrize('mode, s, shape, layout', CASES,
                         ids=[f"{IDS[m]}{s}-{'x'.join(map(str, sh))}-l{lay}" for m, s, sh, lay in CASES])
def test_space_depth_exact(device, dtype, mode, s, shape, layout):
    xb, exp = case(dtype, mode, s, shape, layout)
    check(run(device, desc(dtype, mode, s, shape, layout), xb, exp, dtype), exp, (IDS[mode], s, shape))


@pytest.mark.parametrize('dtype', DT_ALL, ids=['bf16', 'fp16', 'f32', 'fp8'])
@pytest.mark.parametrize('s, shape', [(2, (2, 6, 10, 8)), (3, (1, 9, 6, 24)), (4, (1, 8, 4, 16))])
def test_expand_of_contract_is_the_identity(device, dtype, s, shape):
    xb, mid = case(dtype, C, s, shape, 0)
    got_mid = run(device, desc(dtype, C, s, shape, 0), xb, mid, dtype)
    in_off, in_extra, out_off, out_extra = LAYOUTS[0]
    n, h, w, c = shape
    # Expand reads Contract's output where it lies (its slice at out_off) and writes a slice at in_off
    d = L.DepthDesc()
    d.n, d.h, d.w, d.c, d.in_c_off, d.in_c_stride = n, h // s, w // s, c * s * s, out_off, c * s * s + out_extra
    d.ho, d.wo, d.out_c_off, d.out_c_stride = h, w, in_off, c + in_extra
    d.gain, d.mode, d.dtype = s, E, dtype
    exp = np.full(xb.shape, SENTINEL[dtype], xb.dtype)
    exp[..., in_off:in_off + c] = xb[..., in_off:in_off + c]
    check(run(device, d, got_mid, exp, dtype), exp, ('identity', s, shape))


def test_space_depth_grid_stride_wraps(device):
    """2^20 16-byte vectors on a launch capped at 2^19 lanes: every lane takes two trips of the loop."""
    mode, s, shape, layout = BIG
    xb, exp = case(L.DT_F32, mode, s, shape, layout)
    assert exp[..., :1].size * (shape[3] * s * s // 4) == 1 << 20 > 2048 * 256
    check(run(device, desc(L.DT_F32, mode, s, shape, layout), xb, exp, L.DT_F32), exp, 'grid-stride')


def test_space_depth_statuses(device):
    """Every BAD_ARG and UNSUPPORTED descriptor of tests/test_depth_plan.py with device pointers: the status
    comes back and the output buffer keeps its sentinel (no launch)."""
    x = torch.zeros(1 << 16, dtype=torch.uint8, device=device)
    y = torch.full((1 << 16,), 0x44, dtype=torch.uint8, device=device)
    st = L.stream_handle(device)
    for want, descs in ((L.YCX_ERR_BAD_ARG, bad_descs()), (L.YCX_ERR_UNSUPPORTED, unsupported_descs())):
        for d in descs:
            assert L.lib.ycx_space_depth(ctypes.byref(d), x.data_ptr(), y.data_ptr(), st) == want
    good = sdesc()
    assert L.lib.ycx_space_depth(ctypes.byref(good), None, y.data_ptr(), st) == L.YCX_ERR_BAD_ARG
    assert L.lib.ycx_space_depth(ctypes.byref(good), x.data_ptr(), None, st) == L.YCX_ERR_BAD_ARG
    assert L.lib.ycx_space_depth(ctypes.byref(good), y.data_ptr(), y.data_ptr(), st) == L.YCX_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert bool((y == 0x44).all())
    # ... and the good one runs
    assert L.lib.ycx_space_depth(ctypes.byref(good), x.data_ptr(), y.data_ptr(), st) == L.YCX_OK
    torch.cuda.synchronize()
