"""RobustConv2 on the GPU: ycx_deconv2d and the wide-stride depthwise shapes of ycx_conv2d_grouped bit for
bit on exactly representable operands (the exact-operand bar of tests/test_gpu_conv_exact.py and
tests/test_gpu_gconv.py, whose helpers this file uses), then the rc2-mini config (tests/rc2_case.py)
through Model.forward against the reference's own eval outputs (tests/golden/g8_rc2.npz).

ycx_deconv2d: s in {2, 4, 8} x {bf16, fp16, f32}; n 2 on 5 x 3 (odd, smaller than any tile) and 17 x 9
(306 pixels: crosses the 128-pixel tile twice), cin in {8, 40} (below one 32-wide MFMA K step, and across
one with a ragged tail), cout in {8, 72} (s*s*cout rows: below the 128-row tile and across it, with an
8-row vector tail). Every case reads its input from channel 8 of a buffer 24 wider and writes its output
at channel 16 of a buffer 24 wider, the other channels holding a sentinel that must survive. Reference:
torch's float64 ``F.conv_transpose2d`` on the CPU, rounded once (helpers.rne); act none and leaky 0.125.
K = cin is 8 or 40, so the operand grids (x in steps of 4 / 2^lx within +-4, w in steps of 2 / 2^lw within
+-2) are the finest the element type holds under the span bound K * 2^lx * 2^lw < 2^20 (DGRID).

Depthwise (k 7, s 4) and (k 11, s 8): 13 x 9 and 16 x 16 inputs, 8 and 40 channels (below one 32-channel
chunk, and a full one plus a ragged one), with and without a residual; K = 49 / 121.

The rounded / tie shares (>= 10 % / >= 1 %, from the float64 reference alone) are asserted per
(element type, op, stride) over the shapes of that group -- the smallest maps have 64 outputs, too few
for a share of their own; tests/test_rc2_plan.py checks every group without a GPU.

SiLU: the bar of test_gpu_conv_exact.test_silu_ulps through its own check (check_silu: bit-exact away
from rounding boundaries, within one element-ulp everywhere), fp32 within 4 ulps as in
test_gpu_gconv.test_grouped_silu_ulps."""
import ctypes
import functools
import json
import math
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rc2_case as C
import test_gpu_gconv as T
from helpers import dyadic, elt_ulps, rel_err, rne, rounding_stats, sd_hash
from test_gpu_p6 import TOL
from ycx.utils.synth import synthetic_images

L = pytest.importorskip("ycx._lib")
from ycx.engine import pack_deconv_weights  # noqa: E402
from ycx.nets.yolo import Model  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
TDT, DTYPES, ACTS = T.TDT, T.DTYPES, T.ACTS
SENTINEL, IN_OFF, OUT_OFF, EXTRA = T.SENTINEL, T.IN_OFF, T.OUT_OFF, T.EXTRA

# ---- ycx_deconv2d ----
DECONV_S = (2, 4, 8)
DECONV_MAPS = [(5, 3), (17, 9)]
DECONV_CIN, DECONV_COUT = (8, 40), (8, 72)
# (lx, lw) per (16-bit element type, K = cin); fp32 runs the bf16 operands
DGRID = {L.DT_BF16: {8: (7, 7), 40: (7, 7)}, L.DT_F16: {8: (8, 8), 40: (7, 7)}}


@functools.lru_cache(maxsize=None)
def deconv_operands(dtype, s, h, w, cin, cout, seed=0, grid=None):
    """Operands of one transposed conv (shared by every act that runs it; never modified): x_full
    [n][h][w][cin + 24] NHWC float64 (the slice at channel 8, SENTINEL around it), wt [cin][cout][s][s]
    (torch's layout), b [cout] and the exact pre-activation z [n][cout][h s][w s]. CPU only."""
    n = 2
    lx, lw, xm, wm = grid or (DGRID[L.DT_BF16 if dtype == L.DT_F32 else dtype][cin] + (T.X_MAX, T.W_MAX))
    assert cin * 2 ** lx * 2 ** lw < T.SPAN
    g = torch.Generator().manual_seed(1000 * seed + 131 * cin + 17 * cout + 7 * s + h)
    o = types.SimpleNamespace(dtype=dtype, s=s, h=h, w=w, n=n, cin=cin, cout=cout, ho=h * s, wo=w * s)
    o.x_full = torch.full((n, h, w, cin + EXTRA), SENTINEL, dtype=torch.float64)
    o.x_full[..., IN_OFF:IN_OFF + cin] = dyadic((n, h, w, cin), -xm, xm, xm / 2 ** lx, g)
    o.wt = dyadic((cin, cout, s, s), -wm, wm, wm / 2 ** lw, g)
    o.b = dyadic((cout,), -T.B_MAX, T.B_MAX, T.B_STEP, g)
    for t in (o.x_full, o.wt):  # the element type holds the operands exactly
        assert torch.equal(t.to(TDT[dtype]).double(), t)
    o.z = F.conv_transpose2d(o.x_full[..., IN_OFF:IN_OFF + cin].permute(0, 3, 1, 2), o.wt, o.b, stride=s)
    assert tuple(o.z.shape) == (n, cout, o.ho, o.wo)
    return o


def deconv_desc(o, act=L.ACT_NONE, slope=0.0):
    d = L.ConvDesc()
    d.n, d.h, d.w, d.cin, d.in_c_off, d.in_c_stride = o.n, o.h, o.w, o.cin, IN_OFF, o.cin + EXTRA
    d.ho, d.wo, d.cout, d.cout_pad, d.out_c_off, d.out_c_stride = o.ho, o.wo, o.cout, o.cout, OUT_OFF, o.cout + EXTRA
    d.kh = d.kw = d.stride = o.s
    d.pad, d.act, d.leaky_slope, d.dtype, d.out_layout = 0, act, slope, o.dtype, L.OUT_NHWC
    return d


def deconv_launch(device, o, act=L.ACT_NONE, slope=0.0):
    """One transposed conv through the C ABI; the raw output buffer (SENTINEL-filled before the launch)."""
    tdt = TDT[o.dtype]
    d = deconv_desc(o, act, slope)
    y = torch.full((o.n, o.ho, o.wo, o.cout + EXTRA), SENTINEL, dtype=tdt)
    xd, wd = o.x_full.to(tdt).to(device), pack_deconv_weights(o.wt, tdt).to(device)
    bd, yd = o.b.float().to(device), y.to(device)
    L.check(L.lib.ycx_deconv2d(ctypes.byref(d), xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), yd.data_ptr(),
                               L.stream_handle(device)), "ycx_deconv2d")
    torch.cuda.synchronize()
    return yd.cpu()


def deconv_cases(dtype, s):
    return [deconv_operands(dtype, s, h, w, cin, cout) for h, w in DECONV_MAPS for cin in DECONV_CIN
            for cout in DECONV_COUT]


def group_stats(refs, tdt, what):
    """The input conditions of a group of cases, from their float64 references alone: fp32 holds every
    sum; 16-bit: >= 10 % of the group's outputs need rounding and >= 1 % are exact ties."""
    if tdt == torch.float32:
        for r in refs:
            assert torch.equal(r.float().double(), r), f"{what}: fp32 does not hold the exact sums"
        return None
    stats = [(r.numel(),) + rounding_stats(r, tdt) for r in refs]
    total = sum(n for n, _, _ in stats)
    rounded, ties = sum(n * a for n, a, _ in stats) / total, sum(n * b for n, _, b in stats) / total
    assert rounded >= T.MIN_ROUNDED and ties >= T.MIN_TIES, \
        f"{what}: inputs too easy, {rounded:.3f} of the outputs need rounding, {ties:.3f} are ties"
    return rounded, ties


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('s', DECONV_S)
def test_exact_deconv(device, s, dtype):
    """Both maps x cin {8, 40} x cout {8, 72}, act none and leaky 0.125, input and output as interior
    channel slices: RNE(true sum) in the slice, the sentinel everywhere else."""
    tdt = TDT[dtype]
    cases = deconv_cases(dtype, s)
    for act, slope in ACTS:
        group_stats([T.apply_act(o.z, act, slope) for o in cases], tdt, f"deconv s{s} dtype {dtype} act {act}")
        for o in cases:
            what = f"deconv s{s} {o.h}x{o.w} cin {o.cin} cout {o.cout} dtype {dtype} act {act}"
            T.assert_bits(deconv_launch(device, o, act, slope), T.expected(T.apply_act(o.z, act, slope), tdt), what)


def deconv_silu_operands(dtype, s, h, w, cin, cout):
    """As test_gpu_gconv.silu_operands: z of a few units."""
    hx = min(4.0, 2.0 ** math.floor(math.log2(12 / math.sqrt(cin))))
    return deconv_operands(dtype, s, h, w, cin, cout, seed=3, grid=(3, 3, hx, 1.0))


DECONV_SILU = [(L.DT_BF16, 2, 17, 9, 40, 72), (L.DT_F16, 4, 17, 9, 40, 72), (L.DT_F32, 8, 5, 3, 40, 72)]


def check_silu_slice(got, o, cout, tdt, what):
    """The SiLU bar on the output slice of a raw buffer: sentinel outside, then check_silu (16-bit) or
    4 fp32 ulps (the parity epilogue v / (1 + expf(-v)): expf 1 ulp, the add and the division 2^-24 each)."""
    from test_gpu_conv_exact import SILU_MAX_Z, check_silu
    assert float(o.z.abs().max()) <= SILU_MAX_Z
    assert torch.equal(got[..., :OUT_OFF], torch.full_like(got[..., :OUT_OFF], SENTINEL))
    assert torch.equal(got[..., OUT_OFF + cout:], torch.full_like(got[..., OUT_OFF + cout:], SENTINEL))
    body = got[..., OUT_OFF:OUT_OFF + cout].contiguous()
    if tdt == torch.float32:
        zz = o.z.permute(0, 2, 3, 1)
        ulps = elt_ulps(body, rne(zz / (1 + torch.exp(-zz)), tdt), tdt).abs()
        print(f"\nfp32 SiLU {what}: max {int(ulps.max())} ulps")
        assert int(ulps.max()) <= 4
    else:  # check_silu takes the raw framed buffer and holds the sentinel around the slice to its bits too
        check_silu(got, o.z, L.ACT_SILU, tdt, what, lead=OUT_OFF, tail=got.shape[3] - OUT_OFF - cout)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype,s,h,w,cin,cout', DECONV_SILU)
def test_deconv_silu_ulps(device, dtype, s, h, w, cin, cout):
    o = deconv_silu_operands(dtype, s, h, w, cin, cout)
    check_silu_slice(deconv_launch(device, o, L.ACT_SILU, 0.0), o, cout, TDT[dtype], f"deconv s{s} dtype {dtype}")


# ---- depthwise stride 4 and 8 (ycx_conv2d_grouped) ----
DW_KS = [(7, 4), (11, 8)]
DW_MAPS = [(13, 9), (16, 16)]
DW_C = (8, 40)
DW_GRID = {L.DT_BF16: {49: (7, 7), 121: (6, 7)}, L.DT_F16: {49: (7, 7), 121: (6, 7)}}  # K * 2^lx * 2^lw < 2^20


@functools.lru_cache(maxsize=None)
def dw_operands(dtype, k, s, h, w, c):
    """test_gpu_gconv.operands for a depthwise conv of c channels (its launch / expected take the result)."""
    K, n = k * k, 2
    lx, lw = DW_GRID[L.DT_BF16 if dtype == L.DT_F32 else dtype][K]
    assert K * 2 ** lx * 2 ** lw < T.SPAN
    g = torch.Generator().manual_seed(31 * K + 7 * s + h + 1000 * c)
    o = types.SimpleNamespace(dtype=dtype, cin_g=1, k=k, s=s, h=h, w=w, n=n, C=c, groups=c)
    o.x_full = torch.full((n, h, w, c + EXTRA), SENTINEL, dtype=torch.float64)
    o.x_full[..., IN_OFF:IN_OFF + c] = dyadic((n, h, w, c), -T.X_MAX, T.X_MAX, T.X_MAX / 2 ** lx, g)
    o.wt = dyadic((c, 1, k, k), -T.W_MAX, T.W_MAX, T.W_MAX / 2 ** lw, g)
    o.b = dyadic((c,), -T.B_MAX, T.B_MAX, T.B_STEP, g)
    for t in (o.x_full, o.wt):
        assert torch.equal(t.to(TDT[dtype]).double(), t)
    o.z = F.conv2d(o.x_full[..., IN_OFF:IN_OFF + c].permute(0, 3, 1, 2), o.wt, o.b, s, k // 2, groups=c)
    o.ho, o.wo = o.z.shape[2:]
    return o


def dw_cases(dtype, k, s):
    return [dw_operands(dtype, k, s, h, w, c) for h, w in DW_MAPS for c in DW_C]


def dw_residual(o):
    return dyadic((o.n, o.ho, o.wo, o.C), -4, 4, 1 / 16, torch.Generator().manual_seed(o.k * o.C + o.s + o.h))


def dw_refs(dtype, k, s, residual):
    """[(operands, residual or None, float64 reference)] of one (dtype, k, s) group: leaky 0.125, and with
    ``residual`` the epilogue's exact add."""
    out = []
    for o in dw_cases(dtype, k, s):
        r = dw_residual(o) if residual else None
        ref = T.apply_act(o.z, L.ACT_LEAKY, 0.125)
        out.append((o, r, ref + r.permute(0, 3, 1, 2) if residual else ref))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('residual', [False, True])
@pytest.mark.parametrize('k,s', DW_KS)
def test_exact_depthwise_wide_stride(device, k, s, residual, dtype):
    tdt = TDT[dtype]
    refs = dw_refs(dtype, k, s, residual)
    group_stats([ref for _, _, ref in refs], tdt, f"depthwise k{k} s{s} dtype {dtype} residual {residual}")
    for o, r, ref in refs:
        what = f"depthwise k{k} s{s} {o.h}x{o.w} c {o.C} dtype {dtype} residual {residual}"
        T.assert_bits(T.launch(device, o, L.ACT_LEAKY, 0.125, residual=r), T.expected(ref, tdt), what)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('k,s', DW_KS)
def test_depthwise_wide_stride_nan_reaches_its_windows_only(device, k, s, dtype):
    """One input pixel of image 0 set to NaN (every channel): the outputs whose k x k window holds that
    pixel are NaN, every other output keeps its exact value, the sentinels survive."""
    tdt = TDT[dtype]
    base = dw_operands(dtype, k, s, 16, 16, 40)
    py, px = 9, 6
    o = types.SimpleNamespace(**vars(base))
    o.x_full = base.x_full.clone()
    o.x_full[0, py, px, IN_OFF:IN_OFF + o.C] = float('nan')
    got = T.launch(device, o)
    hit = torch.zeros(o.n, o.ho, o.wo, dtype=torch.bool)
    for oy in range(o.ho):
        for ox in range(o.wo):
            hit[0, oy, ox] = (oy * s - k // 2 <= py < oy * s - k // 2 + k) and (ox * s - k // 2 <= px < ox * s - k // 2 + k)
    assert 0 < int(hit.sum()) < hit.numel() // 2
    body = got[..., OUT_OFF:OUT_OFF + o.C]
    assert torch.equal(torch.isnan(body), hit.unsqueeze(-1).expand_as(body))
    exp = T.expected(base.z, tdt)
    clean = torch.where(torch.isnan(got), exp, got)  # the NaN outputs are accounted for above
    T.assert_bits(clean, exp, f"depthwise k{k} s{s} dtype {dtype} around a NaN")


# ---- the rc2-mini config end to end ----
@pytest.fixture(scope='module')
def g8():
    with open(os.path.join(GOLD, 'g8_rc2.json')) as f:
        meta = json.load(f)
    return meta, dict(np.load(os.path.join(GOLD, 'g8_rc2.npz')))


def rc2_model(precision, meta):
    m = Model(C.rc2_mini(), C.ANCHORS2, C.NC, precision=precision).eval()
    sd = C.state_dict(m)
    assert sd_hash(sd) == meta['sd_hash']  # the fixture's weights, regenerated
    m.load_state_dict(sd)
    return m


@pytest.mark.gpu
@pytest.mark.parametrize('precision', ['f32', 'fp16', 'bf16'])
def test_rc2_mini_vs_reference(device, g8, precision):
    """Bars: TOL of tests/test_gpu_p6.py (f32 1e-3, fp16 1e-3, bf16 2.5e-2), what tests/test_gpu_grouped.py
    holds gx-mini to; max |gpu - ref| / max |ref| per output tensor."""
    meta, gold = g8
    m = rc2_model(precision, meta).to(device)
    x = synthetic_images(*C.SHAPE, seed=C.IMG_SEED)
    assert np.array_equal(x.numpy(), gold['x'])
    x = x.to(device)
    z, xs = m(x)
    assert len(xs) == 2 and [C.SHAPE[2] / t.shape[2] for t in xs] == C.STRIDES
    errs = {'z': rel_err(z.cpu(), torch.from_numpy(gold['z']))}
    for j, t in enumerate(xs):
        g = torch.from_numpy(gold[f'x{j}'])
        assert tuple(t.shape) == tuple(g.shape)
        errs[f'x{j}'] = rel_err(t.cpu(), g)
    print(f"\n{precision} G8 rc2-mini rel err {errs}")
    assert max(errs.values()) < TOL[precision], errs
    eng = m.engine_for(x.shape, device, slot=m.EAGER_SLOT)
    kinds = [i['kind'] for i in eng.op_info]
    assert kinds.count('deconv') == 3 and kinds.count('gconv') == 3 and kinds.count('copy') == 0
    dec = [eng.ops[i].d.conv for i in range(eng.n_ops) if eng.ops[i].kind == L.OP_DECONV]
    assert [(d.stride, d.out_c_off, d.out_c_stride) for d in dec] == [(2, 0, 128), (4, 32, 128), (8, 64, 128)]


@pytest.mark.gpu
@pytest.mark.parametrize('precision', ['bf16', 'fp16'])
def test_rc2_graph_replay_matches_eager(device, g8, precision):
    meta, _ = g8
    m = rc2_model(precision, meta).to(device)
    x = synthetic_images(*C.SHAPE, seed=C.IMG_SEED).to(device)
    eng = m.engine_for(x.shape, device)
    eager = [o.clone() for o in eng.run(x)]
    eng.bind_static(x)
    eng.capture()
    first = [o.clone() for o in eng.replay()]
    torch.cuda.synchronize()
    second = eng.replay()
    torch.cuda.synchronize()
    for a, b, c in zip(eager, first, second):
        assert torch.equal(a, b) and torch.equal(b, c)


@pytest.mark.gpu
def test_rc2_prepack_roundtrip(device, g8, tmp_path):
    """Transposed-conv weights go through the prepack file as [s*s][cout][cin] in the plan's dtype: saved,
    loaded into a freshly initialised module, the forward is bit-identical."""
    meta, _ = g8
    m = rc2_model('bf16', meta).to(device)
    x = synthetic_images(*C.SHAPE, seed=C.IMG_SEED).to(device)
    ref = [o.clone() for o in m.engine_for(x.shape, device).run(x)]
    path = str(tmp_path / 'rc2.safetensors')
    m.save_prepacked(path, C.SHAPE[2:], device=device)
    eng = m.engine_for(x.shape, device)
    kinds = [nd.kind for nd in eng.graph.nodes if nd.kind in ('conv', 'stem', 'stem_reorg', 'gconv', 'deconv')]
    di = [i for i, k in enumerate(kinds) if k == 'deconv']
    assert [tuple(eng.packed[f'p{2 * i}'].shape) for i in di] == [(4, 32, 32), (16, 32, 32), (64, 32, 32)]
    assert all(eng.packed[f'p{2 * i}'].dtype == torch.bfloat16 for i in di)
    m2 = Model(C.rc2_mini(), C.ANCHORS2, C.NC, precision='bf16').eval().to(device)  # random weights
    m2.load_prepacked(path)
    for a, b in zip(ref, m2.engine_for(x.shape, device).run(x)):
        assert torch.equal(a, b)
