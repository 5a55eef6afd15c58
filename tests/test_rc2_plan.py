"""Host-side (CPU) checks of the RobustConv2 work: the builder against the reference's bookkeeping
(tests/golden/g8_rc2.json), the 'deconv' graph node, gamma folding, FLOP accounting, the refused
nn.ConvTranspose2d forms, the fp8 refusal, the argument validation of ycx_deconv2d and of the widened
ycx_conv2d_grouped (no device call is made) and the operand grids of tests/test_gpu_rc2.py."""
import ctypes
import hashlib
import json
import os

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import rc2_case as C
from ycx import _lib as L
from ycx.engine import Graph, Plan, Val, check_plan_precision, fold_robustconv2, lower_module, pack_deconv_weights
from ycx.nets.common import RobustConv2
from ycx.nets.yolo import Model

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope='module')
def g8():
    with open(os.path.join(GOLD, 'g8_rc2.json')) as f:
        return json.load(f)


def test_rc2_mini_parses_like_the_reference(g8):
    m = Model(C.rc2_mini(), C.ANCHORS2, C.NC)
    sd = m.state_dict()
    book = dict(n_layers=len(m.model), save=list(m.save), n_params=sum(p.numel() for p in m.parameters()),
                n_keys=len(sd), keys_sha256=hashlib.sha256('\n'.join(sorted(sd.keys())).encode()).hexdigest())
    assert book == {k: g8[k] for k in book}
    keys = [k[len('model.1.'):] for k in sd if k.startswith('model.1.')]
    assert sorted(keys) == sorted(['conv_strided.conv.weight', 'conv_strided.bn.weight', 'conv_strided.bn.bias',
                                   'conv_strided.bn.running_mean', 'conv_strided.bn.running_var',
                                   'conv_strided.bn.num_batches_tracked', 'conv_deconv.weight', 'conv_deconv.bias',
                                   'gamma'])
    assert g8['min_abs_gamma'] > 0.25  # the fixture's layer scales are O(1), not the 1e-6 init


def test_plan_counts_and_slices():
    plan = Plan(Model(C.rc2_mini(), C.ANCHORS2, C.NC).eval(), C.SHAPE)
    c = plan.counts()
    assert (c['stem'], c['gconv'], c['deconv'], c['conv'], c['copy'], c['concat']) == (1, 3, 3, 5, 0, 1)
    dec = [nd for nd in plan.graph.nodes if nd.kind == 'deconv']
    cat = next(nd for nd in plan.graph.nodes if nd.kind == 'concat')
    assert [(nd.p['s'], nd.inputs[0].h, nd.out.h, nd.out.coff) for nd in dec] == [(2, 32, 64, 0), (4, 16, 64, 32),
                                                                                   (8, 8, 64, 64)]
    for nd in dec:  # written straight into the concat buffer, fed by the strided depthwise conv
        assert nd.out.buf is cat.out.buf and nd.p['layout'] == L.OUT_NHWC and nd.p.get('parts', 1) == 1
        g = nd.inputs[0].producer
        assert g.kind == 'gconv' and (g.p['k'], g.p['s']) in C.RC2 and g.p['groups'] == 32


def test_conv_flops_by_hand():
    """Per image: 2 * ho * wo * cout * cin_g * k * k for a conv, 2 * h * w * cin * s * s * cout for a
    transposed conv on an h x w map."""
    convs = [(64 * 64, 32, 3, 3),                                                  # 0
             (32 * 32, 32, 1, 5), (16 * 16, 32, 1, 7), (8 * 8, 32, 1, 11),         # 1-3: conv_strided
             (64 * 64, 32, 32, 1),                                                 # 4
             (32 * 32, 128, 128, 3), (16 * 16, 128, 128, 3),                       # 6, 7
             (32 * 32, 24, 128, 1), (16 * 16, 24, 128, 1)]                         # heads
    deconvs = [(32 * 32, 32, 2, 32), (16 * 16, 32, 4, 32), (8 * 8, 32, 8, 32)]     # 1-3: conv_deconv
    per_image = sum(2 * px * co * ci * k * k for px, co, ci, k in convs) + \
        sum(2 * px * ci * s * s * co for px, ci, s, co in deconvs)
    plan = Plan(Model(C.rc2_mini(), C.ANCHORS2, C.NC).eval(), C.SHAPE)
    assert plan.conv_flops == C.SHAPE[0] * per_image == 857841664


def test_fold_robustconv2_exact():
    """float64 conv_transpose2d with the folded weights equals the module's definition
    (conv_deconv(x) * gamma) to 1e-12; without gamma the weights are the module's own."""
    torch.manual_seed(5)
    m = RobustConv2(16, 24, 7, 4, layer_scale_init_value=0.5).eval()
    with torch.no_grad():
        m.gamma.copy_(torch.randn(24))
        m.conv_deconv.bias.copy_(torch.randn(24))
    x = torch.randn(2, 16, 5, 3, dtype=torch.float64)
    w, b = fold_robustconv2(m)
    with torch.no_grad():
        want = F.conv_transpose2d(x, m.conv_deconv.weight.double(), m.conv_deconv.bias.double(), stride=4) * \
            m.gamma.double().reshape(1, -1, 1, 1)
    assert float((F.conv_transpose2d(x, w, b, stride=4) - want).abs().max()) < 1e-12
    m.gamma = None
    w, b = fold_robustconv2(m)
    assert torch.equal(w, m.conv_deconv.weight.double()) and torch.equal(b, m.conv_deconv.bias.double())
    # the packed form: row (dy * s + dx) * cout + co holds W[:, co, dy, dx]
    wp = pack_deconv_weights(w, torch.float32)
    assert tuple(wp.shape) == (16, 24, 16) and torch.equal(wp[4 * 2 + 3, 5], w[:, 5, 2, 3].float())


def _act_val(c=32, h=8, w=8):
    return Val(1, h, w, c)


def test_bare_conv_transpose_lowers():
    out = lower_module(Graph(), nn.ConvTranspose2d(32, 48, 4, 4), _act_val())
    assert out.producer.kind == 'deconv' and (out.h, out.w, out.c) == (32, 32, 48)
    out = lower_module(Graph(), nn.ConvTranspose2d(32, 32, 2, 2, bias=False), _act_val())
    assert not out.producer.p['b'].any()
    m = Model({'depth_multiple': 1.0, 'width_multiple': 1.0, 'head': [],
               'backbone': [[-1, 1, 'Conv', [32, 3, 1]], [-1, 1, 'nn.ConvTranspose2d', [32, 32, 2, 2]]]},
              C.ANCHORS2, C.NC).eval()
    assert Plan(m, (1, 3, 16, 16)).counts()['deconv'] == 1


@pytest.mark.parametrize('kw,field', [
    (dict(kernel_size=3, stride=2), 'kernel_size'), (dict(kernel_size=4, stride=2, padding=1), 'kernel_size'),
    (dict(kernel_size=2, stride=2, padding=1), 'padding'),
    (dict(kernel_size=4, stride=4, output_padding=1), 'output_padding'),
    (dict(kernel_size=2, stride=2, dilation=2), 'dilation'), (dict(kernel_size=2, stride=2, groups=2), 'groups'),
    (dict(kernel_size=3, stride=3), 'stride'), (dict(kernel_size=16, stride=16), 'stride'),
    (dict(kernel_size=(2, 4), stride=(2, 4)), 'kernel_size')])
def test_refused_conv_transpose_forms_name_their_field(kw, field):
    with pytest.raises(NotImplementedError, match=field):
        lower_module(Graph(), nn.ConvTranspose2d(32, 32, **kw), _act_val())


def test_deconv_on_the_model_input_and_odd_channels_raise():
    with pytest.raises(NotImplementedError, match='model input'):
        lower_module(Graph(), nn.ConvTranspose2d(3, 8, 2, 2), Val(1, 16, 16, 3, role='input'))
    with pytest.raises(NotImplementedError, match='cout 12'):
        lower_module(Graph(), nn.ConvTranspose2d(32, 12, 2, 2), _act_val())


def test_wide_stride_is_depthwise_only():
    from ycx.engine import conv_module
    from ycx.nets.common import Conv
    for k, s, g in [(7, 4, 16), (11, 1, 16), (3, 8, 8)]:  # cin_g 2, 2, 4
        with pytest.raises(NotImplementedError, match=r'cin_g \d+, cout_g \d+, k \d'):
            conv_module(Graph(), Conv(32, 32, k, s, g=g).eval(), _act_val(32, 16, 16))
    out = conv_module(Graph(), Conv(32, 32, 11, 8, g=32).eval(), _act_val(32, 16, 16))
    assert out.producer.kind == 'gconv' and (out.h, out.w) == (2, 2)


def test_fp8_plan_with_deconv_is_refused():
    plan = Plan(Model(C.rc2_mini(), C.ANCHORS2, C.NC).eval(), C.SHAPE)
    with pytest.raises(NotImplementedError, match='transposed conv has no fp8 path'):
        check_plan_precision(plan, 'fp8')
    for p in ('bf16', 'fp16', 'f32'):
        check_plan_precision(plan, p)


def ddesc(cin=32, cout=48, s=4, h=5, w=3):
    d = L.ConvDesc()
    d.n, d.h, d.w, d.cin, d.in_c_off, d.in_c_stride = 2, h, w, cin, 8, cin + 24
    d.kh = d.kw = d.stride = s
    d.ho, d.wo = h * s, w * s
    d.cout, d.cout_pad, d.out_c_off, d.out_c_stride = cout, cout, 16, cout + 24
    d.act, d.dtype, d.out_layout = L.ACT_NONE, L.DT_BF16, L.OUT_NHWC
    return d


def test_deconv_entry_point_validates_before_any_device_call():
    """Every call here must return before a launch: the pointers are host memory."""
    assert L.OP_DECONV == 10 and L.lib.ycx_abi_version() == 9 and L.lib.ycx_struct_size(12) == 0
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)

    def call(d, x=p, w=p, b=p, y=p):
        return L.lib.ycx_deconv2d(ctypes.byref(d) if d is not None else None, x, w, b, y, None)

    assert call(None) == L.YCX_ERR_BAD_ARG
    for null in ('x', 'w', 'b', 'y'):
        assert call(ddesc(), **{null: None}) == L.YCX_ERR_BAD_ARG
    bad = []
    d = ddesc(); d.ho += 1; bad.append(d)                   # ho not h * s
    d = ddesc(); d.wo = d.w; bad.append(d)
    d = ddesc(); d.in_c_off = 32; bad.append(d)             # slice past its stride
    d = ddesc(); d.out_c_stride = 56; bad.append(d)
    d = ddesc(); d.n = 0; bad.append(d)
    d = ddesc(); d.n = -1; bad.append(d)
    for d in bad:
        assert call(d) == L.YCX_ERR_BAD_ARG
    unsupported = []
    d = ddesc(); d.kh = d.kw = 2; unsupported.append(d)     # kh != stride
    d = ddesc(); d.kw = 2; unsupported.append(d)
    unsupported.append(ddesc(s=3))
    unsupported.append(ddesc(s=1))
    unsupported.append(ddesc(s=16))
    d = ddesc(); d.pad = 1; unsupported.append(d)
    d = ddesc(); d.dtype = L.DT_FP8; unsupported.append(d)
    d = ddesc(); d.act = L.ACT_SILU_PS; unsupported.append(d)
    for layout in (L.OUT_NCHW_F32, L.OUT_NHWC_UP2):
        d = ddesc(); d.out_layout = layout; unsupported.append(d)
    d = ddesc(); d.in_pool = 1; unsupported.append(d)
    d = ddesc(); d.k_split = 2; unsupported.append(d)
    d = ddesc(); d.groups = 2; unsupported.append(d)
    unsupported.append(ddesc(cin=36))                       # cin % 8
    unsupported.append(ddesc(cout=44))                      # cout % 8
    d = ddesc(); d.in_c_off = 4; unsupported.append(d)      # not a 16-byte channel vector
    d = ddesc(); d.out_c_off = 4; unsupported.append(d)
    for d in unsupported:
        assert call(d) == L.YCX_ERR_UNSUPPORTED and call(d, y=None) == L.YCX_ERR_UNSUPPORTED
    for dt in (L.DT_BF16, L.DT_F16, L.DT_F32):              # a valid descriptor: groups 0 and 1 both dense
        for g in (0, 1):
            d = ddesc(); d.dtype, d.groups = dt, g
            assert call(d, y=None) == L.YCX_ERR_BAD_ARG     # ... is taken up to the pointer check
    op = L.Op()
    op.kind = L.OP_DECONV  # the executor routes kind 10 to ycx_deconv2d, which rejects the empty descriptor
    assert L.lib.ycx_run_ops(ctypes.byref(op), 1, None, None) == L.YCX_ERR_BAD_ARG
    assert ctypes.sizeof(L.Op) == L.lib.ycx_struct_size(8)


def test_grouped_entry_point_takes_the_wide_depthwise_shapes():
    """(k 7, s 4) and (k 11, s 8) depthwise descriptors pass every check up to the pointer check; a wider
    group, k 9 and s 3 stay unsupported. The entry point judges the descriptor before the data pointers,
    so with a null x a descriptor it takes returns BAD_ARG and one it does not returns UNSUPPORTED: no call
    here reaches a launch."""
    from test_grouped_plan import gdesc
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)

    def call(d, x=p):
        return L.lib.ycx_conv2d_grouped(ctypes.byref(d), x, p, p, p, None, None)

    for k, s in [(7, 4), (11, 8), (11, 1), (3, 8), (5, 4)]:
        for dt in (L.DT_BF16, L.DT_F16, L.DT_F32):
            d = gdesc(k=k, s=s, h=16, w=16); d.dtype = dt
            assert call(d, x=None) == L.YCX_ERR_BAD_ARG
    for d in (gdesc(c=48, g=24, k=11, s=1), gdesc(c=48, g=24, k=7, s=4), gdesc(c=48, g=24, k=3, s=8),
              gdesc(k=9), gdesc(s=3), gdesc(k=11, s=3), gdesc(k=13, s=8)):
        assert call(d) == L.YCX_ERR_UNSUPPORTED and call(d, x=None) == L.YCX_ERR_UNSUPPORTED


def test_exact_case_grids_meet_their_conditions():
    """The operand grids of tests/test_gpu_rc2.py, checked here without a GPU for every group: the span bound
    (asserted in the operand builders), >= 10 % rounded and >= 1 % ties per 16-bit group, lossless fp32
    sums, and the SiLU cases' input conditions -- as test_grouped_plan does for the gconv grids."""
    import test_gpu_rc2 as R
    from test_gpu_conv_exact import SILU_MAX_Z, silu_conditions
    T = R.T
    for dtype in R.DTYPES:
        tdt = R.TDT[dtype]
        for s in R.DECONV_S:
            cases = R.deconv_cases(dtype, s)
            assert len(cases) == 8
            for act, slope in R.ACTS:
                R.group_stats([T.apply_act(o.z, act, slope) for o in cases], tdt, f"deconv s{s} {dtype} {act}")
        for k, s in R.DW_KS:
            for residual in (False, True):
                R.group_stats([ref for _, _, ref in R.dw_refs(dtype, k, s, residual)], tdt, f"dw k{k} s{s} {dtype}")
    for dtype, s, h, w, cin, cout in R.DECONV_SILU:
        o = R.deconv_silu_operands(dtype, s, h, w, cin, cout)
        assert float(o.z.abs().max()) <= SILU_MAX_Z
        if dtype != L.DT_F32:
            silu_conditions(o.z, L.ACT_SILU, R.TDT[dtype], "deconv SiLU")
