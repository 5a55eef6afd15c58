"""Host-side (CPU) checks of the P6 pieces: ReOrg / DownC in the builder, the ``stem_reorg``
lowering and where it is refused, and the new entry point's argument validation."""
import ctypes
import hashlib
import json
import os

import pytest
import torch

import p6_case as P
from ycx.engine import Plan
from ycx.nets.common import Conv
from ycx.nets.yolo import Model, parse_model
from ycx.utils.helper_io import cvt_cfg

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
ANCHORS3 = [[12, 16, 19, 36, 40, 28], [36, 75, 76, 55, 72, 146], [142, 110, 192, 243, 459, 401]]


@pytest.fixture(scope='module')
def g5_meta():
    with open(os.path.join(GOLD, 'g5_p6.json')) as f:
        return json.load(f)


@pytest.mark.parametrize('name', list(P.VARIANTS))
def test_parse_model_matches_the_reference_record(g5_meta, name):
    e = g5_meta[name]
    layers, save = parse_model(P.p6_mini(P.VARIANTS[name]), [3], P.ANCHORS4, P.NC)
    assert len(layers) == e['n_layers'] and save == e['save']
    assert sum(p.numel() for p in layers.parameters()) == e['n_params']
    m = Model(P.p6_mini(P.VARIANTS[name]), P.ANCHORS4, P.NC)
    sd = m.state_dict()
    assert len(sd) == e['n_keys']
    assert hashlib.sha256('\n'.join(sorted(sd.keys())).encode()).hexdigest() == e['keys_sha256']


def _module_flops(model, shape):
    """2 * K * cout * output pixels of every Conv2d the eval forward runs, from the module tree: each
    conv's input map follows from the layer's stride bookkeeping (ReOrg halves the sides first)."""
    n, _, h, w = shape
    total, sizes = 0, []
    for m in model.model:
        f = m.f if isinstance(m.f, int) else m.f[0]
        hw = (h // 2, w // 2) if m.i == 0 else (sizes[f] if f != -1 else sizes[-1])
        name = type(m).__name__
        if name == 'ReOrg':
            out = hw
        elif name == 'Upsample':
            out = (2 * hw[0], 2 * hw[1])
        elif name == 'DownC':
            out = (hw[0] // 2, hw[1] // 2)
            for cv, px in ((m.cv1, hw), (m.cv2, out), (m.cv3, out)):
                c = cv.conv
                total += 2 * n * px[0] * px[1] * c.out_channels * c.in_channels * c.kernel_size[0] ** 2
        elif name in ('IDetect', 'IAuxDetect'):
            for i in range(m.nl):  # the aux heads are never launched
                src = sizes[m.f[i]]
                total += 2 * n * src[0] * src[1] * m.m[i].out_channels * m.m[i].in_channels
            out = hw
        else:  # Conv, SPPCSPC, Concat: every inner conv is 'same' at the layer's output size
            s = m.conv.stride[0] if isinstance(m, Conv) else 1
            out = (hw[0] // s, hw[1] // s)
            for c in (mm for mm in m.modules() if isinstance(mm, torch.nn.Conv2d)):
                total += 2 * n * out[0] * out[1] * c.out_channels * c.in_channels * c.kernel_size[0] ** 2
        sizes.append(out)
    return total


@pytest.mark.parametrize('name', list(P.VARIANTS))
def test_plan_has_one_stem_reorg(name):
    m = Model(P.p6_mini(P.VARIANTS[name]), P.ANCHORS4, P.NC)
    plan = Plan(m, P.SHAPE)
    c = plan.counts()
    assert c.get('stem_reorg') == 1 and 'stem' not in c and c.get('copy', 0) == 0 and c.get('up', 0) == 0
    nd = next(nd for nd in plan.graph.nodes if nd.kind == 'stem_reorg')
    assert (nd.inputs[0].h, nd.inputs[0].w, nd.inputs[0].c) == (64, 64, 12) and tuple(nd.p['w'].shape) == (64, 12, 3, 3)
    assert [(v.h, v.c) for v in plan.out_vals] == [(16, 24), (8, 24), (4, 24), (2, 24)]
    assert plan.conv_flops == _module_flops(m, P.SHAPE)
    assert c['pool'] == 4 + 3  # one k2 pool per DownC, the SPPCSPC 5/9/13 set as three k5 pools


def test_reorg_is_refused_off_the_input_and_before_other_convs():
    d = lambda bb: {'depth_multiple': 1.0, 'width_multiple': 1.0, 'backbone': bb, 'head': []}
    mid = Model(d([[-1, 1, 'Conv', [32, 3, 1]], [-1, 1, 'ReOrg', []], [-1, 1, 'Conv', [64, 3, 1]]]), ANCHORS3, 1)
    with pytest.raises(NotImplementedError, match='only on the model input'):
        Plan(mid, (1, 3, 32, 32))
    k1 = Model(d([[-1, 1, 'ReOrg', []], [-1, 1, 'Conv', [64, 1, 1]]]), ANCHORS3, 1)
    with pytest.raises(NotImplementedError, match='ReOrg'):
        Plan(k1, (1, 3, 32, 32))
    two = Model(d([[-1, 1, 'ReOrg', []], [-1, 1, 'Conv', [64, 3, 1]], [0, 1, 'Conv', [64, 3, 2]]]), ANCHORS3, 1)
    with pytest.raises(NotImplementedError, match='only consumer'):
        Plan(two, (1, 3, 32, 32))
    pooled = Model(d([[-1, 1, 'ReOrg', []], [-1, 1, 'MP', []]]), ANCHORS3, 1)
    with pytest.raises(NotImplementedError, match='ReOrg'):
        Plan(pooled, (1, 3, 32, 32))
    ok = Model(d([[-1, 1, 'ReOrg', []], [-1, 1, 'Conv', [64, 3, 2]]]), ANCHORS3, 1)
    assert Plan(ok, (1, 3, 32, 32)).counts() == {'stem_reorg': 1, 'tonchw': 1}
    for shape in ((1, 3, 33, 32), (1, 3, 32, 31)):
        with pytest.raises(ValueError, match='even image sides'):
            Plan(ok, shape)


def test_shortcut_stays_out_of_scope():
    d = {'depth_multiple': 1.0, 'width_multiple': 1.0, 'backbone': [[-1, 1, 'Shortcut', [1]]], 'head': []}
    with pytest.raises(NotImplementedError, match='out of scope'):
        parse_model(d, [3], ANCHORS3, 1)


def test_yolov7_plan_counts_unchanged():
    plan = Plan(Model(cvt_cfg('yolov7'), ANCHORS3, 80), (2, 3, 640, 640))
    c = plan.counts()
    assert c['stem'] == 1 and c['conv'] + c['stem'] == 92 and 'stem_reorg' not in c
    assert c['merged'] == 8 and c['pool'] == 8
    assert abs(plan.conv_flops / 2 / 1e9 - 104.5110784) < 1e-6


def test_stem_conv_reorg_validates_before_any_device_call():
    """No GPU: null pointers and inconsistent descriptors return before anything is launched."""
    from ycx import _lib as L
    assert 'ycx_stem_conv_reorg' in L.SYMBOLS and L.OP_STEM_REORG == 8 and L.lib.ycx_abi_version() == 9
    f = L.lib.ycx_stem_conv_reorg
    assert f(None, None, None, None, None, None) == L.YCX_ERR_BAD_ARG
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)

    def desc(**kw):
        d = L.ConvDesc()
        d.n, d.h, d.w, d.cin, d.in_c_off, d.in_c_stride = 1, 8, 8, 12, 0, 3
        d.ho, d.wo, d.cout, d.cout_pad, d.out_c_off, d.out_c_stride = 8, 8, 32, 32, 0, 32
        d.kh = d.kw = 3
        d.stride, d.pad, d.dtype, d.out_layout = 1, 1, L.DT_BF16, L.OUT_NHWC
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    for dt in (L.DT_BF16, L.DT_F16, L.DT_F32, L.DT_FP8):
        assert f(ctypes.byref(desc(dtype=dt)), None, p, p, p, None) == L.YCX_ERR_BAD_ARG
        assert f(ctypes.byref(desc(dtype=dt)), p, p, p, None, None) == L.YCX_ERR_BAD_ARG
    for bad in (dict(cin=3), dict(in_c_stride=5, cin=20), dict(in_c_stride=0, cin=0), dict(ho=7), dict(wo=9),
                dict(stride=2), dict(in_c_off=1)):
        assert f(ctypes.byref(desc(**bad)), p, p, p, p, None) == L.YCX_ERR_BAD_ARG, bad
    for unsup in (dict(kh=1, kw=1, pad=0), dict(kh=5, kw=5, pad=2, ho=8, wo=8), dict(pad=0, ho=6, wo=6),
                  dict(stride=4, ho=2, wo=2)):
        assert f(ctypes.byref(desc(**unsup)), p, p, p, p, None) == L.YCX_ERR_UNSUPPORTED, unsup
    op = L.Op()
    op.kind = L.OP_STEM_REORG
    op.d.conv = desc()
    assert L.lib.ycx_run_ops(ctypes.byref(op), 1, None, None) == L.YCX_ERR_BAD_ARG  # null operands, no launch
