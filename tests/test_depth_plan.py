"""Host-side (CPU) checks of the space/depth layers: the builder's Focus / Contract / Expand against the
reference's bookkeeping (tests/golden/g11_depth.json), the 'depth' graph node and its launch, the Expand
output aliased into its concat buffer, Focus on the image as a ``stem_reorg`` node, every refusal with its
message, the modules that stay out of scope, and the C entry point's argument validation (no device call
is made)."""
import ctypes
import hashlib
import json
import os

import pytest

import depth_case as C
from ycx import _lib as L
from ycx.engine import DEPTH_NAME, Graph, Plan, Val, check_plan_precision, lower_module
from ycx.nets.common import Contract, Conv, Expand, Focus
from ycx.nets.yolo import Model, parse_model
from ycx.schedule import Schedule

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
BOOK = ('n_layers', 'save', 'n_params', 'n_keys', 'keys_sha256')


@pytest.fixture(scope='module')
def g11():
    with open(os.path.join(GOLD, 'g11_depth.json')) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def plan():
    return Plan(Model(C.sd_mini(), C.ANCHORS2, C.NC).eval(), C.SHAPE)


def book(m):
    return dict(n_layers=len(m.model), save=list(m.save), n_params=sum(p.numel() for p in m.parameters()),
                n_keys=len(m.state_dict()),
                keys_sha256=hashlib.sha256('\n'.join(sorted(m.state_dict().keys())).encode()).hexdigest())


@pytest.mark.parametrize('name', sorted(C.SINGLES))
def test_depth_modules_parse_like_the_reference(g11, name):
    module, args, c_in, op_name = C.SINGLES[name]
    m = Model(C.single(module, args, c_in), C.ANCHORS2, C.NC)
    assert book(m) == g11['singles'][name]
    p = Plan(m.eval(), C.SINGLE_SHAPE)  # and lowers
    assert p.counts()['depth'] == 1
    la = [la for la in Schedule(p, 'bf16').launches if la.kind == 'depth']
    assert len(la) == 1 and len(la[0].nodes) == 1
    nd = la[0].nodes[0]
    assert f"{DEPTH_NAME[nd.p['mode']]}{nd.p['gain']}" == op_name
    x, y, s = nd.inputs[0], nd.out, nd.p['gain']
    if nd.p['mode'] == L.SD_EXPAND:
        assert (y.n, y.h, y.w, y.c) == (x.n, x.h * s, x.w * s, x.c // (s * s))
    else:
        assert (y.n, y.h, y.w, y.c) == (x.n, x.h // s, x.w // s, x.c * s * s)


@pytest.mark.parametrize('stem, key', [('focus', 'sd_mini'), ('conv', 'sd_mini_conv')])
def test_sd_mini_bookkeeping(g11, stem, key):
    m = Model(C.sd_mini(stem), C.ANCHORS2, C.NC).eval()
    assert book(m) == {k: g11[key][k] for k in BOOK}


def test_reference_state_dict_names():
    """Focus keeps the reference's attribute names: conv.conv.weight over 4 c1 channels, conv.bn.*."""
    f = Focus(16, 64, 3, 1, None, 8)
    assert isinstance(f.conv, Conv) and tuple(f.conv.conv.weight.shape) == (64, 8, 3, 3) and f.conv.conv.groups == 8
    assert sorted(k for k in f.state_dict() if 'num_batches' not in k) == [
        'conv.bn.bias', 'conv.bn.running_mean', 'conv.bn.running_var', 'conv.bn.weight', 'conv.conv.weight']
    assert Contract().gain == 2 and Expand(3).gain == 3 and not Contract(2).state_dict()


def test_sd_mini_plan(plan):
    c = plan.counts()
    assert c['depth'] == C.N_DEPTH and c['stem_reorg'] == 1 and 'stem' not in c
    assert c['copy'] == 0 and c['concat'] == 1 and 'tonchw' not in c
    depth = [nd for nd in plan.graph.nodes if nd.kind == 'depth']
    assert [(nd.p['mode'], nd.p['gain']) for nd in depth] == [(L.SD_CONTRACT, 2), (L.SD_EXPAND, 2), (L.SD_FOCUS, 2)]
    contract, expand, focus = depth
    assert (contract.out.h, contract.out.w, contract.out.c) == (8, 8, 256)
    assert contract.out.consumers[0].kind == 'conv' and contract.out.buf.c == 256
    # the Expand output is written straight into its slice of layer 6's concat buffer: no copy
    cat = next(nd for nd in plan.graph.nodes if nd.kind == 'concat')
    assert cat.inputs[0] is expand.out and cat.p['copies'] == []
    assert expand.out.buf is cat.out.buf and expand.out.coff == 0 and expand.out.c == 32 and cat.out.buf.c == 64
    assert cat.inputs[1].buf is cat.out.buf and cat.inputs[1].coff == 32
    assert (expand.inputs[0].c, expand.out.h, expand.out.w) == (128, 16, 16)
    # the Focus on an activation: the move, then its 1x1 conv over 4 x 64 channels
    assert focus.inputs[0] is cat.out and (focus.out.h, focus.out.w, focus.out.c) == (8, 8, 256)
    fc = focus.out.consumers
    assert len(fc) == 1 and fc[0].kind == 'conv' and tuple(fc[0].p['w'].shape) == (64, 256, 1, 1)
    for prec in ('bf16', 'fp16', 'f32', 'fp8'):
        kinds = [la.kind for la in Schedule(plan, prec).launches]
        assert kinds.count('depth') == C.N_DEPTH and 'copy' not in kinds
        check_plan_precision(plan, prec)  # no precision is refused


def test_conv_stem_variant_plan():
    c = Plan(Model(C.sd_mini('conv'), C.ANCHORS2, C.NC).eval(), C.SHAPE).counts()
    assert c['depth'] == C.N_DEPTH and c['stem'] == 1 and 'stem_reorg' not in c and c['copy'] == 0


def test_focus_on_the_image_is_a_stem_reorg(g11, plan):
    m = Model(C.on_input('Focus', [32, 3]), C.ANCHORS2, C.NC)
    assert book(m) == g11['singles']['Focus_on_input']
    p = Plan(m.eval(), (1, 3, 32, 32))
    assert p.counts() == {'stem_reorg': 1, 'tonchw': 1}
    nd = p.graph.nodes[0]
    assert tuple(nd.p['w'].shape) == (32, 12, 3, 3) and (nd.p['k'], nd.p['s'], nd.p['p']) == (3, 1, 1)
    assert nd.inputs[0].role == 'reorg' and (nd.out.h, nd.out.w, nd.out.c) == (16, 16, 32)
    stem = plan.graph.nodes[0]  # sd-mini's own stem
    assert stem.kind == 'stem_reorg' and (stem.out.h, stem.out.w, stem.out.c) == (32, 32, 32)
    s2 = lower_module(Graph(), Focus(3, 32, 3, 2).eval(), Val(1, 32, 32, 3, role='input'))  # stride 2 is taken too
    assert s2.producer.kind == 'stem_reorg' and (s2.h, s2.w) == (8, 8)


def image():
    return Val(1, 32, 32, 3, role='input')


@pytest.mark.parametrize('args', [(3, 32, 1), (3, 32, 5), (3, 32, 3, 4), (3, 32, 3, 1, 0), (3, 36, 3, 1, None, 3)])
def test_focus_on_the_image_outside_the_stem_kernels_limits(args):
    with pytest.raises(NotImplementedError, match=r'ycx_stem_conv_reorg, which takes a 3x3 / pad-1 conv of stride '
                                                  r'1 or 2 with groups 1'):
        lower_module(Graph(), Focus(*args).eval(), image())


def test_focus_on_an_odd_image_keeps_reorgs_message():
    with pytest.raises(ValueError, match='ReOrg needs even image sides'):
        lower_module(Graph(), Focus(3, 32, 3).eval(), Val(1, 31, 32, 3, role='input'))


def test_depth_node_refusals():
    g = Graph()
    for m in (Contract(2), Expand(2)):  # the image, and a ReOrg view of it
        with pytest.raises(NotImplementedError, match='on the model input'):
            lower_module(g, m, image())
        with pytest.raises(NotImplementedError, match='on the model input'):
            lower_module(g, m, g.reorg(image()))
    with pytest.raises(NotImplementedError, match='on the model input'):
        g.depth(g.reorg(image()), L.SD_FOCUS, 2)
    act = Val(1, 24, 24, 64)
    limits = r'ycx_space_depth takes a gain in \(2, 3, 4\) \(Focus: 2\) and a contiguous channel run'
    for gain in (1, 5, 0, 2.0):
        with pytest.raises(NotImplementedError, match=limits):
            g.depth(act, L.SD_CONTRACT, gain)
        with pytest.raises(NotImplementedError, match=limits):
            g.depth(Val(1, 24, 24, 3600), L.SD_EXPAND, gain)
    with pytest.raises(NotImplementedError, match=limits):
        g.depth(Val(1, 24, 24, 64), L.SD_FOCUS, 4)
    with pytest.raises(NotImplementedError, match=limits):  # a run of 12
        g.depth(Val(1, 24, 24, 12), L.SD_CONTRACT, 2)
    with pytest.raises(NotImplementedError, match=limits):  # 64 / 4 = 16 is a run, 48 / 4 = 12 is not
        g.depth(Val(1, 24, 24, 48), L.SD_EXPAND, 2)
    with pytest.raises(NotImplementedError, match=limits):
        lower_module(g, Focus(4, 32, 1).eval(), Val(1, 24, 24, 4))
    # what the reference's view refuses
    with pytest.raises(ValueError, match='spatial sides divisible by 2'):
        g.depth(Val(1, 24, 23, 64), L.SD_CONTRACT, 2)
    with pytest.raises(ValueError, match='spatial sides divisible by 4'):
        g.depth(Val(1, 22, 24, 64), L.SD_CONTRACT, 4)
    with pytest.raises(ValueError, match='spatial sides divisible by 2'):
        lower_module(g, Focus(64, 64, 1).eval(), Val(1, 7, 8, 64))
    with pytest.raises(ValueError, match='channels divisible by 9'):
        g.depth(Val(1, 24, 24, 64), L.SD_EXPAND, 3)
    out = g.depth(Val(1, 6, 9, 24), L.SD_CONTRACT, 3)
    assert out.producer.kind == 'depth' and (out.h, out.w, out.c) == (2, 3, 216)
    out = g.depth(Val(1, 2, 3, 128), L.SD_EXPAND, 4)
    assert (out.h, out.w, out.c) == (8, 12, 8)


def test_expand_run_of_nine_is_refused():
    with pytest.raises(NotImplementedError, match='a run of 9'):
        Graph().depth(Val(1, 2, 3, 144), L.SD_EXPAND, 4)


def test_reorg_rules_do_not_change():
    from ycx.nets.common import ReOrg
    with pytest.raises(NotImplementedError, match='ReOrg is lowered only on the model input'):
        lower_module(Graph(), ReOrg(), Val(1, 16, 16, 64))
    g = Graph()
    with pytest.raises(NotImplementedError, match=r"ReOrg is lowered only into the Conv .* here a 'pool' reads it"):
        g.pool(g.reorg(image()), 2, 2, 0)


@pytest.mark.parametrize('name', ['Shortcut', 'Stem', 'GhostStem', 'Chuncat', 'Foldcut'])
def test_still_out_of_scope(name):
    with pytest.raises(NotImplementedError, match='out of scope'):
        parse_model(C.single(name, [64]), [3], C.ANCHORS2, C.NC)


def test_fp8_scales_tie_a_depth_ops_buffers(plan):
    """The union-find of Engine._assign_fp8_scales, run here on the plan alone: each depth node's input and
    output buffers land in one group."""
    from ycx.engine import Engine
    bufs = Schedule(plan, 'fp8').activation_bufs
    eng = Engine.__new__(Engine)
    eng.graph, eng.scales = plan.graph, {}
    eng.activation_bufs = lambda: bufs
    # a different amax per buffer: tied buffers must still come out with one scale
    eng._assign_fp8_scales([dict(c=b.c, amax=float(2 ** (i % 7))) for i, b in enumerate(bufs)])
    for nd in plan.graph.nodes:
        if nd.kind == 'depth':
            assert eng.scales[id(nd.inputs[0].buf)] == eng.scales[id(nd.out.buf)]


def sdesc(mode=L.SD_CONTRACT, gain=2, h=6, w=12, c=16):
    d = L.DepthDesc()
    ss = gain * gain
    d.n, d.h, d.w, d.c, d.in_c_off, d.in_c_stride = 2, h, w, c, 8, c + 16
    if mode == L.SD_EXPAND:
        d.ho, d.wo, co = h * gain, w * gain, c // ss
    else:
        d.ho, d.wo, co = h // gain, w // gain, c * ss
    d.out_c_off, d.out_c_stride = 16, co + 24
    d.gain, d.mode, d.dtype = gain, mode, L.DT_BF16
    return d


def bad_descs():
    """Descriptors ycx_space_depth answers with YCX_ERR_BAD_ARG (tests/test_gpu_space_depth.py sends them too)."""
    bad = []
    d = sdesc(); d.n = 0; bad.append(d)
    d = sdesc(h=7); d.ho = 3; bad.append(d)                                  # h % s
    d = sdesc(w=11); d.wo = 5; bad.append(d)                                 # w % s
    d = sdesc(L.SD_FOCUS, w=11); d.wo = 5; bad.append(d)
    d = sdesc(L.SD_CONTRACT, 3, h=6, w=10); bad.append(d)                    # w % 3
    d = sdesc(L.SD_EXPAND, 3, c=64); d.out_c_stride = 64; bad.append(d)      # C % 9
    d = sdesc(L.SD_EXPAND, 2, c=72); d.c = 70; bad.append(d)                 # C % 4
    d = sdesc(); d.ho += 1; bad.append(d)                                    # ho / wo against h, w, s
    d = sdesc(); d.wo = d.w; bad.append(d)
    d = sdesc(L.SD_EXPAND, c=64); d.ho = d.h; bad.append(d)
    d = sdesc(L.SD_EXPAND, c=64); d.wo -= 1; bad.append(d)
    d = sdesc(); d.in_c_off = 24; bad.append(d)                              # a slice past its stride
    d = sdesc(); d.out_c_stride = 72; bad.append(d)
    d = sdesc(L.SD_EXPAND, c=64); d.out_c_stride = 24; bad.append(d)
    d = sdesc(); d.in_c_off = -8; bad.append(d)
    return bad


def unsupported_descs():
    """... and with YCX_ERR_UNSUPPORTED."""
    unsupported = []
    for gain in (0, 1, 5, 8):
        d = sdesc(); d.gain = gain; unsupported.append(d)
    d = sdesc(L.SD_FOCUS, 3, h=6, w=12); unsupported.append(d)               # Focus with s != 2
    d = sdesc(L.SD_FOCUS, 4, h=8, w=12); unsupported.append(d)
    d = sdesc(c=12); unsupported.append(d)                                   # a run of 12
    d = sdesc(L.SD_EXPAND, c=48); d.out_c_stride = 40; unsupported.append(d)  # a run of 12
    d = sdesc(L.SD_EXPAND, 3, c=36); d.out_c_stride = 32; unsupported.append(d)  # a run of 4
    d = sdesc(); d.in_c_off = 4; unsupported.append(d)                       # not multiples of 8
    d = sdesc(); d.in_c_stride = 36; unsupported.append(d)
    d = sdesc(); d.out_c_off = 20; unsupported.append(d)
    d = sdesc(); d.out_c_stride = 92; unsupported.append(d)
    d = sdesc(); d.dtype = 4; unsupported.append(d)
    d = sdesc(); d.dtype = -1; unsupported.append(d)
    d = sdesc(); d.mode = 3; unsupported.append(d)
    d = sdesc(); d.mode = -1; unsupported.append(d)
    return unsupported


def test_space_depth_entry_point_validates_before_any_device_call():
    """Every call here must return before a launch: the pointers are host memory."""
    assert L.OP_DEPTH == 12 and L.ABI_VERSION == 9 and L.lib.ycx_abi_version() == 9
    assert 'ycx_space_depth' in L.SYMBOLS
    assert ctypes.sizeof(L.Op) == L.lib.ycx_struct_size(8) and L.lib.ycx_struct_size(12) == 0
    assert ctypes.sizeof(L.DepthDesc) == 13 * 4 <= ctypes.sizeof(L.ConvDesc) * 2
    buf, other = (ctypes.c_char * 64)(), (ctypes.c_char * 64)()
    p, q = ctypes.addressof(buf), ctypes.addressof(other)

    def call(d, x=p, y=q):
        return L.lib.ycx_space_depth(ctypes.byref(d) if d is not None else None, x, y, None)

    assert call(None) == L.YCX_ERR_BAD_ARG
    assert call(L.DepthDesc()) == L.YCX_ERR_BAD_ARG  # the empty descriptor
    for mode, gain, c in ((L.SD_CONTRACT, 2, 16), (L.SD_CONTRACT, 3, 16), (L.SD_FOCUS, 2, 16), (L.SD_EXPAND, 2, 64),
                          (L.SD_EXPAND, 4, 128)):
        for null in ('x', 'y'):  # a null pointer with a good descriptor
            assert call(sdesc(mode, gain, c=c), **{null: None}) == L.YCX_ERR_BAD_ARG
    for d in bad_descs():
        assert call(d) == L.YCX_ERR_BAD_ARG
    # x == y: only slices of one pixel stride with disjoint channel ranges
    d = sdesc()                                                              # different pixel strides
    assert call(d, x=p, y=p) == L.YCX_ERR_BAD_ARG
    d = sdesc(); d.in_c_off, d.in_c_stride, d.out_c_off, d.out_c_stride = 72, 96, 16, 96   # [72, 88) meets [16, 80)
    assert call(d, x=p, y=p) == L.YCX_ERR_BAD_ARG
    for d in unsupported_descs():
        assert call(d) == L.YCX_ERR_UNSUPPORTED
    # the descriptor is judged first: a null pointer with an unsupported one reports the descriptor
    d = sdesc(); d.gain = 5
    assert call(d, x=None) == L.YCX_ERR_UNSUPPORTED
    op = L.Op()
    op.kind = L.OP_DEPTH  # the executor routes kind 12 to ycx_space_depth, which rejects the empty descriptor
    assert L.lib.ycx_run_ops(ctypes.byref(op), 1, None, None) == L.YCX_ERR_BAD_ARG
    op.d.depth = sdesc(); op.d.depth.gain = 7  # ... and reads d.depth
    assert L.lib.ycx_run_ops(ctypes.byref(op), 1, None, None) == L.YCX_ERR_UNSUPPORTED


def test_existing_schedules_hold_no_depth_launch():
    """No yolov7 plan contains a depth node: the schedule golden of the shipped configs lists none."""
    with open(os.path.join(GOLD, 'g7_schedule.json')) as f:
        assert '"depth"' not in f.read()
