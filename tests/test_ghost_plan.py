"""Host-side (CPU) checks of the Ghost family: the builder's new module names against the reference's
bookkeeping (tests/golden/g9_ghost.json), the 'ghost' graph node, its in-place placement and its
residual, the modules that stay out of scope, the refused shapes, the fp8 refusal, the C entry point's
argument validation (no device call is made) and the operand table of tests/test_gpu_ghost_dw.py."""
import ctypes
import hashlib
import json
import os

import pytest
import torch

import ghost_case as C
from ycx import _lib as L
from ycx.engine import Graph, Plan, Val, check_plan_precision, lower_module
from ycx.nets.common import Ghost, GhostConv
from ycx.nets.yolo import Model, parse_model

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope='module')
def g9():
    with open(os.path.join(GOLD, 'g9_ghost.json')) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def plan():
    return Plan(Model(C.gh_mini(), C.ANCHORS2, C.NC).eval(), C.SHAPE)


def book(m):
    return dict(n_layers=len(m.model), save=list(m.save), n_params=sum(p.numel() for p in m.parameters()),
                n_keys=len(m.state_dict()),
                keys_sha256=hashlib.sha256('\n'.join(sorted(m.state_dict().keys())).encode()).hexdigest())


@pytest.mark.parametrize('name', sorted(C.SINGLES))
def test_ghost_modules_parse_like_the_reference(g9, name):
    module, args, c_in = C.SINGLES[name]
    m = Model(C.single(module, args, c_in), C.ANCHORS2, C.NC)
    assert book(m) == g9['singles'][name]
    p = Plan(m.eval(), (1, 3, 32, 32))  # and lowers
    assert p.counts()['ghost'] >= 1


def test_gh_mini_bookkeeping(g9):
    m = Model(C.gh_mini(), C.ANCHORS2, C.NC).eval()
    want = {k: g9['gh_mini'][k] for k in ('n_layers', 'save', 'n_params', 'n_keys', 'keys_sha256')}
    assert book(m) == want


def test_gh_mini_plan(plan):
    c = plan.counts()
    assert c['ghost'] == C.N_GHOST and c['gconv'] == C.N_GCONV and c['stem'] == 1
    assert c['copy'] == 0 and c['up'] == 1  # the only copy kernel is the upsample under layer 10's GhostConv
    ghosts = [nd for nd in plan.graph.nodes if nd.kind == 'ghost']
    with_res = [nd for nd in ghosts if nd.p['residual'] is not None]
    assert len(with_res) == C.N_GHOST_RES
    for nd in ghosts:
        y, out = nd.inputs[0], nd.out
        assert out.c == 2 * y.c and y.c % 8 == 0 and nd.p['k'] == 5 and nd.p['layout'] == L.OUT_NHWC
        assert y.producer.kind in ('conv', 'gconv')  # cv1 stays an ordinary node
        if nd.p['residual'] is None:  # in place: cv1 stores y into the first half of the ghost's output
            assert y.buf is out.buf and y.coff == out.coff, "a residual-free ghost op must run in place"
            assert nd.p['act'] == L.ACT_SILU
        else:                         # the first half is y + r: y keeps a buffer of its own
            assert y.buf is not out.buf and nd.inputs[1] is nd.p['residual']
            assert nd.p['residual'].c == out.c and nd.p['act'] == L.ACT_NONE
    # layer 12's Ghost writes its slice of layer 13's concat buffer; layer 10 feeds the unfused upsample
    cat = next(nd for nd in plan.graph.nodes if nd.kind == 'concat' and nd.out.c == 256 and nd.out.h == 16)
    assert cat.inputs[0].producer.kind == 'ghost' and cat.inputs[0].buf is cat.out.buf and cat.p['copies'] == []
    up = next(nd for nd in plan.graph.nodes if nd.kind == 'up')
    assert up.inputs[0].producer.kind == 'ghost' and up.out.buf is cat.out.buf and up.out.coff == 128
    # the s = 2 Ghost: its residual is the shortcut's 1x1 conv, and both depthwise 3x3 / s2 are 'gconv' nodes
    s2 = [nd for nd in with_res if nd.p['residual'].producer.kind == 'conv' and nd.out.c == 256]
    assert len(s2) == 1 and s2[0].inputs[0].producer.inputs[0].producer.kind == 'gconv'


def test_ghost_flops(plan):
    """A ghost node counts its depthwise conv: 2 * N * H * W * c * 25."""
    nodes = plan.graph.nodes
    ghost = sum(2 * nd.out.n * nd.out.h * nd.out.w * nd.inputs[0].c * 25 for nd in nodes if nd.kind == 'ghost')
    assert ghost > 0
    rest = sum(2 * nd.inputs[0].n * nd.p['ho'] * nd.p['wo'] * int(nd.p['w'].shape[0]) * int(nd.p['w'].shape[1])
               * nd.p['k'] ** 2 for nd in nodes if nd.kind in ('conv', 'stem', 'gconv'))
    assert plan.conv_flops == ghost + rest


@pytest.mark.parametrize('name', sorted(C.SINGLES))
def test_ghost_family_on_the_model_input_is_out_of_scope(name):
    module, args, _ = C.SINGLES[name]
    with pytest.raises(NotImplementedError, match='out of scope'):
        parse_model(C.on_input(module, args), [3], C.ANCHORS2, C.NC)


@pytest.mark.parametrize('name', ['Shortcut', 'Stem', 'GhostStem', 'Chuncat', 'Foldcut'])
def test_still_out_of_scope(name):
    with pytest.raises(NotImplementedError, match='out of scope'):
        parse_model(C.single(name, [64]), [3], C.ANCHORS2, C.NC)


def test_refused_shapes():
    with pytest.raises(NotImplementedError, match=r'c % 8 == 0'):  # hidden width 12
        lower_module(Graph(), GhostConv(32, 24, 1, 1).eval(), Val(1, 16, 16, 32))
    odd = GhostConv(32, 32, 1, 1).eval()
    odd.cv2 = type(odd.cv2)(16, 16, 3, 1, None, 16)  # cv2 is not the depthwise 5x5
    with pytest.raises(NotImplementedError, match='depthwise 5x5'):
        lower_module(Graph(), odd, Val(1, 16, 16, 32))
    with pytest.raises(ValueError, match='c1 == c2'):  # the reference's add fails there
        lower_module(Graph(), Ghost(64, 128, 3, 1).eval(), Val(1, 16, 16, 64))
    with pytest.raises(NotImplementedError, match='model input'):
        lower_module(Graph(), GhostConv(3, 32, 1, 1).eval(), Val(1, 16, 16, 3, role='input'))
    out = lower_module(Graph(), Ghost(64, 64, 3, 1).eval(), Val(1, 16, 16, 64))
    assert out.producer.kind == 'ghost' and (out.h, out.w, out.c) == (16, 16, 64)


def test_fp8_plan_with_ghost_is_refused(plan):
    with pytest.raises(NotImplementedError, match='ghost conv has no fp8 path'):
        check_plan_precision(plan, 'fp8')
    for p in ('bf16', 'fp16', 'f32'):
        check_plan_precision(plan, p)


def hdesc(c=48, h=13, w=11):
    d = L.ConvDesc()
    d.n, d.h, d.w, d.cin, d.in_c_off, d.in_c_stride = 2, h, w, c, 8, c + 24
    d.kh = d.kw = 5
    d.stride, d.pad, d.ho, d.wo = 1, 2, h, w
    d.cout, d.cout_pad, d.out_c_off, d.out_c_stride = 2 * c, 2 * c, 16, 2 * c + 24
    d.act, d.dtype, d.out_layout, d.groups = L.ACT_NONE, L.DT_BF16, L.OUT_NHWC, c
    return d


def test_ghost_entry_point_validates_before_any_device_call():
    """Every call here must return before a launch: the pointers are host memory."""
    assert L.OP_GHOST == 11 and L.ABI_VERSION == 9
    buf, other = (ctypes.c_char * 64)(), (ctypes.c_char * 64)()
    p, q = ctypes.addressof(buf), ctypes.addressof(other)

    def call(d, x=p, w=p, b=p, y=q, r=None):
        return L.lib.ycx_ghost_dw(ctypes.byref(d) if d is not None else None, x, w, b, y, r, None)

    assert call(None) == L.YCX_ERR_BAD_ARG
    for null in ('x', 'w', 'b', 'y'):  # a null pointer with a good descriptor
        assert call(hdesc(), **{null: None}) == L.YCX_ERR_BAD_ARG
    bad = []
    d = hdesc(); d.ho = 7; bad.append(d)                    # ho not implied by h, k, s, pad
    d = hdesc(); d.wo += 1; bad.append(d)
    d = hdesc(); d.in_c_off = 32; bad.append(d)             # slice past its stride
    d = hdesc(); d.out_c_stride = 104; bad.append(d)
    d = hdesc(); d.n = 0; bad.append(d)
    for d in bad:
        assert call(d) == L.YCX_ERR_BAD_ARG
    d = hdesc(); d.res_c_off, d.res_c_stride = 8, 96          # the residual slice is 2c wide
    assert call(d, r=p) == L.YCX_ERR_BAD_ARG
    # in place (x == y, the same slice) takes no residual; other intersecting slices of one buffer are refused
    d = hdesc(); d.in_c_off, d.in_c_stride = d.out_c_off, d.out_c_stride
    d.res_c_off, d.res_c_stride = 0, 96
    assert call(d, x=p, y=p, r=q) == L.YCX_ERR_BAD_ARG
    d = hdesc(); d.in_c_off, d.in_c_stride = 24, d.out_c_stride  # [24, 72) meets [16, 112)
    assert call(d, x=p, y=p) == L.YCX_ERR_BAD_ARG
    d = hdesc()                                                # same pointer, different pixel strides
    assert call(d, x=p, y=p) == L.YCX_ERR_BAD_ARG
    unsupported = []
    d = hdesc(); d.kh = d.kw = 3; d.pad = 1; unsupported.append(d)           # k 3
    d = hdesc(); d.stride = 2; d.ho, d.wo = 7, 6; unsupported.append(d)      # stride 2
    d = hdesc(); d.pad = 0; d.ho, d.wo = 9, 7; unsupported.append(d)         # pad != 2
    d = hdesc(); d.cout = 48; unsupported.append(d)                          # cout != 2 cin
    d = hdesc(); d.groups = 24; unsupported.append(d)                        # not depthwise
    d = hdesc(); d.dtype = L.DT_FP8; unsupported.append(d)
    d = hdesc(); d.act = L.ACT_SILU_PS; unsupported.append(d)
    d = hdesc(); d.out_layout = L.OUT_NHWC_UP2; unsupported.append(d)
    d = hdesc(); d.in_pool = 1; unsupported.append(d)
    d = hdesc(); d.k_split = 2; unsupported.append(d)
    d = hdesc(); d.in_c_off = 4; unsupported.append(d)                       # not a multiple of 8
    d = hdesc(c=44); unsupported.append(d)                                   # c % 8
    for d in unsupported:
        assert call(d) == L.YCX_ERR_UNSUPPORTED
    # the descriptor is judged first: a null pointer with an unsupported one reports the descriptor
    d = hdesc(); d.dtype = L.DT_FP8
    assert call(d, x=None) == L.YCX_ERR_UNSUPPORTED
    op = L.Op()
    op.kind = L.OP_GHOST  # the executor routes kind 11 to ycx_ghost_dw, which rejects the empty descriptor
    assert L.lib.ycx_run_ops(ctypes.byref(op), 1, None, None) == L.YCX_ERR_BAD_ARG


def test_exact_case_table_meets_its_conditions():
    """The operand table of tests/test_gpu_ghost_dw.py, checked here without a GPU: per case and per half at
    least 10 % of the outputs need rounding and at least 1 % are exact ties (16-bit), fp32 holds every value
    exactly, and the SiLU cases meet their input conditions."""
    import test_gpu_ghost_dw as T
    from test_gpu_conv_exact import SILU_MAX_Z, silu_conditions
    for dtype in T.DTYPES:
        for hw in T.MAPS:
            for c in T.CS:
                o = T.gh_operands(dtype, c, *hw)
                assert (o.n, o.C, o.k, o.s) == (2, c, 5, 1) and tuple(o.z.shape) == (2, c, *hw)
                r = T.residual_of(o)
                assert torch.equal(r.to(T.TDT[dtype]).double(), r) and torch.equal(r * 1024, (r * 1024).round())
                for act, slope in T.ACTS:
                    T.check_case(o, act, slope)
                    T.check_case(o, act, slope, r)
        o = T.silu_operands(dtype)
        assert float(o.z.abs().max()) <= SILU_MAX_Z
        if dtype != L.DT_F32:
            silu_conditions(o.z, L.ACT_SILU, T.TDT[dtype], "ghost SiLU")
