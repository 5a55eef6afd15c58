"""Host-side (CPU) checks of the grouped-conv work: the builder's new module names against the
reference's bookkeeping (tests/golden/g6_grouped.json), the 'gconv' graph node and the passes that
must leave it alone, FLOP accounting, RobustConv folding, the rejected shapes, the fp8 refusal and
the C entry point's argument validation (no device call is made)."""
import ctypes
import hashlib
import json
import os

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import grouped_case as C
from ycx import _lib as L
from ycx.engine import Graph, Plan, Val, check_plan_precision, conv_module, fold_bn, fold_robustconv, lower_module
from ycx.nets.common import Conv, RobustConv
from ycx.nets.yolo import Model

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope='module')
def g6():
    with open(os.path.join(GOLD, 'g6_grouped.json')) as f:
        return json.load(f)


def book(m):
    return dict(n_layers=len(m.model), save=list(m.save), n_params=sum(p.numel() for p in m.parameters()),
                n_keys=len(m.state_dict()),
                keys_sha256=hashlib.sha256('\n'.join(sorted(m.state_dict().keys())).encode()).hexdigest())


@pytest.mark.parametrize('name', sorted(C.SINGLES))
def test_new_modules_parse_like_the_reference(g6, name):
    module, args, c_in = C.SINGLES[name]
    m = Model(C.single(module, args, c_in), C.ANCHORS2, C.NC)
    assert book(m) == g6['singles'][name]
    Plan(m.eval(), (1, 3, 32, 32))  # and lowers


def test_gx_mini_bookkeeping_and_plan(g6):
    m = Model(C.gx_mini(), C.ANCHORS2, C.NC).eval()
    want = {k: g6['gx_mini'][k] for k in ('n_layers', 'save', 'n_params', 'n_keys', 'keys_sha256')}
    assert book(m) == want
    plan = Plan(m, C.SHAPE)
    c = plan.counts()
    assert c['gconv'] == C.N_GCONV and c['copy'] == 0 and c['up'] == 1 and c['stem'] == 1
    gnodes = [nd for nd in plan.graph.nodes if nd.kind == 'gconv']
    assert sorted(int(nd.p['w'].shape[1]) for nd in gnodes) == [1, 1, 1, 1, 2, 4, 16]
    for nd in gnodes:  # not merged, not upsample-fused; the pairing / pool passes look for kind 'conv'
        assert nd.p.get('parts', 1) == 1 and nd.p['layout'] == L.OUT_NHWC and nd.p['groups'] > 1
    # layer 4's depthwise conv writes its slice of layer 5's concat buffer; layer 13 feeds the unfused upsample
    dw5 = next(nd for nd in gnodes if nd.p['k'] == 5)
    cat = next(nd for nd in plan.graph.nodes if nd.kind == 'concat' and dw5.out in nd.inputs)
    assert dw5.out.buf is cat.out.buf and dw5.out.coff == 0 and cat.p['copies'] == []
    up = next(nd for nd in plan.graph.nodes if nd.kind == 'up')
    assert up.inputs[0].producer.kind == 'gconv'
    assert sum(1 for nd in gnodes if nd.p['residual'] is not None) == 1  # Bottleneck g = 4


def test_conv_flops_by_hand():
    """2 * ho * wo * cout * cin_g * k * k per image (a dense conv: cin_g = cin), layer by layer."""
    t16, t8 = 16 * 16, 8 * 8
    terms = [
        (64 * 64, 32, 3, 3), (32 * 32, 64, 32, 3), (t16, 64, 1, 3), (t16, 64, 64, 1), (t16, 64, 1, 5),  # 0-4
        (t16, 64, 128, 1), (t16, 64, 2, 3), (t16, 128, 64, 1),                                          # 6 ResX
        (t8, 128, 128, 3),                                                                             # 7
        (t8, 128, 128, 1), (t8, 128, 128, 1), (t8, 128, 4, 3), (t8, 128, 128, 1), (t8, 128, 128, 1),    # 8 ResXCSPC
        (t8, 128, 128, 1), (t8, 256, 256, 1),
        (t8, 64, 256, 1), (t8, 32, 64, 1), (t8, 32, 32, 3), (t8, 64, 32, 1), (t8, 64, 256, 1),          # 9 ResCSPA
        (t8, 128, 128, 1),
        (t8, 64, 128, 1), (t8, 64, 64, 1), (t8, 64, 16, 3),                                            # 10, 11
        (t8, 64, 1, 7), (t8, 128, 64, 1), (t8, 128, 1, 3),                                             # 12, 13
        (t16, 128, 256, 1), (t16, 128, 128, 3), (t16, 24, 128, 1), (t8, 24, 128, 1),                   # 16, 17, heads
    ]
    per_image = sum(2 * px * co * ci * k * k for px, co, ci, k in terms)
    plan = Plan(Model(C.gx_mini(), C.ANCHORS2, C.NC).eval(), C.SHAPE)
    assert plan.conv_flops == C.SHAPE[0] * per_image == 403881984


def test_fold_robustconv_exact():
    """float64 conv2d with the folded 1x1 equals the module's definition (conv1x1(y) * gamma) to 1e-12."""
    torch.manual_seed(3)
    m = RobustConv(16, 24, 7, 1, layer_scale_init_value=0.5).eval()
    with torch.no_grad():
        m.gamma.copy_(torch.randn(24))
        m.conv1x1.bias.copy_(torch.randn(24))
    y = torch.randn(2, 16, 9, 7, dtype=torch.float64)
    w, b = fold_robustconv(m)
    with torch.no_grad():
        want = F.conv2d(y, m.conv1x1.weight.double(), m.conv1x1.bias.double()) * m.gamma.double().reshape(1, -1, 1, 1)
    assert float((F.conv2d(y, w, b) - want).abs().max()) < 1e-12
    m.gamma = None
    w, b = fold_robustconv(m)
    assert torch.equal(w, m.conv1x1.weight.double()) and torch.equal(b, m.conv1x1.bias.double())
    # the depthwise half folds its BN like any Conv
    wd, bd = fold_bn(m.conv_dw.conv.weight, m.conv_dw.bn)
    assert tuple(wd.shape) == (16, 1, 7, 7) and tuple(bd.shape) == (16,)


def _act_val(c=48):
    v = Val(1, 16, 16, c)
    return v


@pytest.mark.parametrize('c1,c2,k,g,what', [(48, 48, 3, 16, 'cin_g 3'), (32, 64, 3, 4, 'cin_g 8, cout_g 16'),
                                            (48, 48, 1, 48, 'k 1'), (64, 64, 3, 2, 'cin_g 32')])
def test_unsupported_grouped_shapes_raise(c1, c2, k, g, what):
    m = Conv(c1, c2, k, 1, g=g).eval()
    with pytest.raises(NotImplementedError, match=r'cin_g \d+, cout_g \d+, k \d'):
        conv_module(Graph(), m, _act_val(c1))


def test_dilation_and_input_grouped_conv_raise():
    m = Conv(48, 48, 3, 1, g=48).eval()
    m.conv.dilation = (2, 2)
    with pytest.raises(NotImplementedError, match='dilated'):
        conv_module(Graph(), m, _act_val())
    bare = nn.Conv2d(48, 48, 3, 1, 1, dilation=2, groups=48)
    with pytest.raises(NotImplementedError, match='dilated'):
        lower_module(Graph(), bare, _act_val())
    with pytest.raises(NotImplementedError, match='model input'):
        conv_module(Graph(), Conv(3, 3, 3, 1, g=3).eval(), Val(1, 16, 16, 3, role='input'))
    out = lower_module(Graph(), nn.Conv2d(48, 48, 5, 2, 2, groups=48), _act_val())  # a bare grouped nn.Conv2d lowers
    assert out.producer.kind == 'gconv' and (out.h, out.w, out.c) == (8, 8, 48)


def test_fp8_plan_with_gconv_is_refused():
    plan = Plan(Model(C.gx_mini(), C.ANCHORS2, C.NC).eval(), C.SHAPE)
    with pytest.raises(NotImplementedError, match='grouped conv has no fp8 path'):
        check_plan_precision(plan, 'fp8')
    for p in ('bf16', 'fp16', 'f32'):
        check_plan_precision(plan, p)
    from helpers import ANCHORS
    from ycx.utils.helper_io import cvt_cfg
    check_plan_precision(Plan(Model(cvt_cfg('yolov7-tiny'), ANCHORS, 1).eval(), (1, 3, 64, 64)), 'fp8')  # dense: fine


def gdesc(c=48, g=48, k=3, s=1, h=13, w=11):
    d = L.ConvDesc()
    d.n, d.h, d.w, d.cin, d.in_c_off, d.in_c_stride = 2, h, w, c, 8, c + 24
    d.kh = d.kw = k
    d.stride, d.pad = s, k // 2
    d.ho, d.wo = (h + 2 * d.pad - k) // s + 1, (w + 2 * d.pad - k) // s + 1
    d.cout, d.cout_pad, d.out_c_off, d.out_c_stride = c, c, 16, c + 24
    d.act, d.dtype, d.out_layout, d.groups = L.ACT_NONE, L.DT_BF16, L.OUT_NHWC, g
    return d


def test_grouped_entry_point_validates_before_any_device_call():
    """Every call here must return before a launch: the pointers are host memory."""
    assert L.OP_GCONV == 9
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)

    def call(d, x=p, w=p, b=p, y=p, r=None):
        return L.lib.ycx_conv2d_grouped(ctypes.byref(d) if d is not None else None, x, w, b, y, r, None)

    assert call(None) == L.YCX_ERR_BAD_ARG
    for null in ('x', 'w', 'b', 'y'):
        assert call(gdesc(), **{null: None}) == L.YCX_ERR_BAD_ARG
    bad = []
    d = gdesc(); d.ho = 7; bad.append(d)                    # ho not implied by h, k, s, pad
    d = gdesc(); d.wo += 1; bad.append(d)
    d = gdesc(); d.in_c_off = 32; bad.append(d)             # slice past its stride
    d = gdesc(); d.out_c_stride = 56; bad.append(d)
    d = gdesc(g=5); bad.append(d)                           # cin % groups != 0
    d = gdesc(); d.n = 0; bad.append(d)
    for d in bad:
        assert call(d) == L.YCX_ERR_BAD_ARG
    d = gdesc(); d.res_c_off, d.res_c_stride = 8, 48         # residual slice past its stride
    assert call(d, r=p) == L.YCX_ERR_BAD_ARG
    unsupported = []
    unsupported.append(gdesc(g=16))                          # cin_g 3
    unsupported.append(gdesc(c=64, g=2))                     # cin_g 32
    unsupported.append(gdesc(g=1))                           # dense
    d = gdesc(); d.cout, d.out_c_stride = 96, 120; unsupported.append(d)   # cin_g != cout_g
    unsupported.append(gdesc(k=1))
    unsupported.append(gdesc(k=9))
    unsupported.append(gdesc(s=3))
    d = gdesc(); d.pad = 0; d.ho, d.wo = 11, 9; unsupported.append(d)      # pad != k / 2
    d = gdesc(); d.dtype = L.DT_FP8; unsupported.append(d)
    d = gdesc(); d.act = L.ACT_SILU_PS; unsupported.append(d)
    d = gdesc(); d.out_layout = L.OUT_NHWC_UP2; unsupported.append(d)
    d = gdesc(); d.in_pool = 1; unsupported.append(d)
    d = gdesc(); d.k_split = 2; unsupported.append(d)
    d = gdesc(); d.in_c_off = 4; unsupported.append(d)       # not a 16-byte channel vector
    d = gdesc(c=44, g=44); unsupported.append(d)             # cout % 8
    for d in unsupported:
        assert call(d) == L.YCX_ERR_UNSUPPORTED
    # the dense entry points refuse a grouped descriptor
    d = L.ConvDesc()
    d.n, d.h, d.w, d.cin, d.in_c_stride, d.ho, d.wo, d.cout, d.cout_pad, d.out_c_stride = 1, 8, 8, 64, 64, 8, 8, 64, 64, 64
    d.kh = d.kw = d.stride = 1
    d.groups = 2
    assert L.lib.ycx_conv2d(ctypes.byref(d), p, p, p, p, None, None) == L.YCX_ERR_UNSUPPORTED
    assert L.lib.ycx_stem_conv(ctypes.byref(d), p, p, p, p, None) == L.YCX_ERR_UNSUPPORTED
    assert L.lib.ycx_stem_conv_reorg(ctypes.byref(d), p, p, p, p, None) == L.YCX_ERR_UNSUPPORTED
    assert L.lib.ycx_conv2d_pair(ctypes.byref(d), ctypes.byref(d), p, p, p, p, p, p, p, None) == L.YCX_ERR_UNSUPPORTED
    op = L.Op()
    op.kind = L.OP_GCONV  # the executor routes kind 9 to the grouped entry point, which rejects the empty descriptor
    assert L.lib.ycx_run_ops(ctypes.byref(op), 1, None, None) == L.YCX_ERR_BAD_ARG


def test_exact_case_grids_meet_their_conditions():
    """The operand grids of tests/test_gpu_gconv.py, checked here without a GPU for the whole grid: the
    span bound (asserted in ``operands``), >= 10 % rounded and >= 1 % ties per 16-bit case, lossless fp32
    sums, and the SiLU cases' input conditions."""
    import test_gpu_gconv as T
    from helpers import dyadic
    from test_gpu_conv_exact import SILU_MAX_Z, silu_conditions
    for dtype in T.DTYPES:
        tdt = T.TDT[dtype]
        for cin_g in T.CIN_GS:
            for k in T.KS:
                for s in T.STRIDES:
                    for h, w in T.maps(s):
                        o = T.operands(dtype, cin_g, k, s, h, w)
                        for act, slope in T.ACTS:
                            T.check_inputs(T.apply_act(o.z, act, slope), tdt, f"{dtype} {cin_g} {k} {s} {h}x{w} {act}")
        for cin_g, k, s in T.RES_CASES:
            o = T.operands(dtype, cin_g, k, s, 13, 11)
            r = dyadic((o.n, o.ho, o.wo, o.C), -4, 4, 1 / 16, torch.Generator().manual_seed(cin_g * k + s))
            T.check_inputs(T.apply_act(o.z, L.ACT_LEAKY, 0.125) + r.permute(0, 3, 1, 2), tdt, "residual")
    for dtype, cin_g, k, s in [(L.DT_BF16, 1, 3, 1), (L.DT_F16, 4, 5, 2), (L.DT_F32, 2, 3, 1)]:
        o = T.silu_operands(dtype, cin_g, k, s)
        assert float(o.z.abs().max()) <= SILU_MAX_Z
        if dtype != L.DT_F32:
            silu_conditions(o.z, L.ACT_SILU, T.TDT[dtype], "grouped SiLU")
