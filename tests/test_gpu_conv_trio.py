"""ycx_conv2d_pair_pool: the 1x1 pair (tile 55) plus the MP branch's 1x1 on the k2 s2 max-pool of
the first map, one launch over tiles of two image rows x 32 columns.

Shapes (n, h, w), the smallest at which each mechanism can go wrong:
  (1, 2, 32)    1 tile: most blocks return early
  (3, 6, 96)    27 tiles: image boundaries, a tile count that is no multiple of anything
  (2, 64, 160)  320 tiles > the 256-block grid: the ring crosses tile boundaries inside a block and
                the counted waits see the stores of all three outputs
"""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from helpers import SENTINEL, make_model
from trio_case import YA_OFF, YB_OFF, YC_OFF, TrioCase
from ycx import _lib as L
from ycx.utils.synth import synthetic_images

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DBG = os.path.join(REPO, "yolo-continuous_amd", "ycx", "libycx_hip_dbg.so")

S1, S2, S3 = (1, 2, 32), (3, 6, 96), (2, 64, 160)
N, PS, LK = L.ACT_NONE, L.ACT_SILU_PS, L.ACT_LEAKY
# (shape, cin, cout_b, cout_c, acts (a, b, c), ya stored): cin 64 / 128 / 256, cout_b_pad 128 / 256,
# each act in each position, ya given and null, cout < cout_pad (the uncounted-wait path) on every shape
CASES = [
    (S1, 64, 128, 128, (N, N, N), True),
    (S1, 128, 248, 120, (PS, PS, PS), False),
    (S2, 256, 128, 128, (LK, LK, LK), True),
    (S2, 64, 256, 120, (PS, LK, N), False),
    (S3, 256, 128, 128, (PS, PS, PS), False),   # yolov7 layers 11 / 14 / 13
    (S3, 128, 120, 128, (LK, PS, LK), True),
    (S3, 256, 256, 128, (N, LK, PS), True),
]


def _ref_act(v, act):
    """float64 activation of a pre-activation v as the kernels define it (YCX_ACT_SILU_PS: v = k c)."""
    if act == L.ACT_NONE:
        return v
    if act == L.ACT_LEAKY:
        return F.leaky_relu(v, 0.1)
    c = v / L.SILU_PS_K
    return c * torch.sigmoid(c)


@pytest.mark.parametrize('dtype', [L.DT_BF16, L.DT_F16])
@pytest.mark.parametrize('shape,cin,cout_b,cout_c,acts,store_a', CASES)
def test_conv2d_pair_pool(device, dtype, shape, cin, cout_b, cout_c, acts, store_a):
    """y2 and y3 (and y1 when stored) of the fused launch are bit-identical to ycx_conv2d_pair followed
    by ycx_conv2d with in_pool = 1 on the stored y1; nothing is written outside the channel slices: each
    output is the interior slice of a sentinel-filled buffer, the sentinel must stand before and behind it
    in the fused and in the unfused buffers (the padding rows of w_b / w_c are live), x lies between NaN
    channels and NaN guards, and no output holds a NaN.
    On (3, 6, 96) y3 also agrees with a float64 conv of the max-pooled 16-bit y1, at
    test_conv2d_pair's tolerance (1e-2 bf16, 2e-3 fp16)."""
    case = TrioCase(device, dtype, shape, cin, cout_b, cout_c, acts)
    ya0, yb0, yc0 = case.unfused()
    ya, yb, yc = case.fused(store_a)
    assert torch.equal(yb, yb0)
    assert torch.equal(yc, yc0)
    if store_a:
        assert torch.equal(ya, ya0)
    else:
        assert bool((ya == SENTINEL).all())
    for name, t, off, c in (('ya', ya, YA_OFF, 256), ('yb', yb, YB_OFF, cout_b), ('yc', yc, YC_OFF, cout_c),
                            ('ya0', ya0, YA_OFF, 256), ('yb0', yb0, YB_OFF, cout_b), ('yc0', yc0, YC_OFF, cout_c)):
        assert t.shape[3] > off + c, name  # a non-empty tail
        assert bool((t[..., :off] == SENTINEL).all()) and bool((t[..., off + c:] == SENTINEL).all()), \
            f"{name}: wrote outside the channel slice"
        assert not bool(t.isnan().any()), f"{name}: something outside the operands reached the output"
    body = yc0[..., YC_OFF:YC_OFF + cout_c]
    assert bool((body != SENTINEL).any()) and bool((yb0[..., YB_OFF:YB_OFF + cout_b] != SENTINEL).any())
    if shape == S2:
        h = case.host
        y1 = ya0[..., YA_OFF:YA_OFF + 256].cpu().double().permute(0, 3, 1, 2)
        pre = F.conv2d(F.max_pool2d(y1, 2, 2), h['wc'][:cout_c].double()[:, :, None, None], h['bc'][:cout_c].double())
        ref = _ref_act(pre, acts[2]).permute(0, 2, 3, 1)
        tol = 1e-2 if dtype == L.DT_BF16 else 2e-3
        torch.testing.assert_close(yc[..., YC_OFF:YC_OFF + cout_c].cpu().double(), ref, rtol=tol, atol=tol)


def test_conv2d_pair_pool_rejects(device):
    """h odd, w % 32 != 0, c->in_pool == 0, c->cin != 256 and c->cout_pad != 128 are unsupported:
    the status comes back before any launch (the outputs keep their sentinel)."""
    def edit(case, what):
        if what == 'h_odd':
            case.da.h = case.da.ho = case.db.h = case.db.ho = 3
            case.dc.h = case.dc.ho = 1
        elif what == 'w_not_32':
            case.da.w = case.da.wo = case.db.w = case.db.wo = 16
            case.dc.w = case.dc.wo = 8
        elif what == 'no_pool':
            case.dc.in_pool = 0
        elif what == 'cin_c':
            case.dc.cin = 128
        elif what == 'cpad_c':
            case.dc.cout_pad = 256
    for what in ('h_odd', 'w_not_32', 'no_pool', 'cin_c', 'cpad_c'):
        case = TrioCase(device, L.DT_BF16, (1, 4, 32), 64, 128, 128, (N, N, N), cpad_c=256 if what == 'cpad_c' else 128)
        edit(case, what)
        ya, yb, yc = case.outputs()
        assert case.fused_status(ya, yb, yc) == L.YCX_ERR_UNSUPPORTED, what
        torch.cuda.synchronize()
        assert all(bool((t == SENTINEL).all()) for t in (ya, yb, yc)), what


def _names(eng):
    return [(i['kind'], i['name'], i.get('parts', 1)) for i in eng.op_info]


def test_plan_yolov7_pair_pool(device):
    """yolov7 bf16 at bs 8 / 640^2: one conv_pair op of three parts (layers 11, 14, 13), four of the
    five MP pools left in pooled convs of their own, outputs bit-identical to the plan with
    fuse_pair_pool=False. At bs 2 (no pair) the plan is the same either way."""
    from ycx.engine import Engine
    m, _ = make_model('yolov7', 80, 0, 'bf16')
    m.to(device)
    dev = torch.device(device)
    x = synthetic_images(8, 3, 640, 640, seed=6).to(device)
    outs = []
    for fuse in (True, False):
        eng = Engine(m, tuple(x.shape), dev, 'bf16', fuse_pair_pool=fuse)
        try:
            pairs = [i for i in eng.op_info if i['kind'] == 'conv_pair']
            assert len(pairs) == 1 and pairs[0]['parts'] == (3 if fuse else 2)
            assert pairs[0]['shape'][1:5] == (160, 160, 256, 256)
            assert not pairs[0]['name'].endswith('+maxpool_k2s2')
            assert sum(1 for i in eng.op_info if i['name'].endswith('+maxpool_k2s2')) == (4 if fuse else 5)
            if fuse:
                fused_bytes, fused_flops = pairs[0]['bytes'], pairs[0]['flops']
            else:  # y1's write and its read are gone from the fused op's bytes; the flops are the sum
                mp = next(i for i in eng.op_info if i['name'].endswith('+maxpool_k2s2'))
                y1 = 8 * 160 * 160 * 256 * 2
                assert fused_bytes == pairs[0]['bytes'] + mp['bytes'] - 2 * y1
                assert fused_flops == pairs[0]['flops'] + mp['flops']
            outs.append([o.clone() for o in eng.run(x)])
        finally:
            eng.close()
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    plans = []
    for fuse in (True, False):
        eng = Engine(m, (2, 3, 640, 640), dev, 'bf16', fuse_pair_pool=fuse)
        plans.append(_names(eng))
        eng.close()
    assert plans[0] == plans[1] and not any(k == 'conv_pair' for k, _, _ in plans[0])


@pytest.mark.parametrize('shape', [(1, 3, 640, 640), (8, 3, 640, 640), (32, 3, 320, 320)])
def test_plan_yolov7_tiny_unchanged(device, shape):
    from ycx.engine import Engine
    m, _ = make_model('yolov7-tiny', 80, 0, 'bf16')
    m.to(device)
    plans = []
    for fuse in (True, False):
        eng = Engine(m, shape, torch.device(device), 'bf16', fuse_pair_pool=fuse)
        plans.append(_names(eng))
        eng.close()
    assert plans[0] == plans[1] and not any(p == 3 for _, _, p in plans[0])


def test_pair_pool_debug_bounds():
    """One fused launch per shape on the bounds-check build: no store outside the three outputs."""
    if not os.path.exists(DBG):
        pytest.skip("libycx_hip_dbg.so not built (opt-in: YCX_BUILD_DEBUG=1 build()): make -C yolo-continuous_amd/csrc debug")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "probes", "bounds_trio.py")],
                       env=dict(os.environ, YCX_LIB=DBG), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["runs"] == 3 and res["violations"] == 0 and res["equal"], res
