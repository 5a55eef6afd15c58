"""Host-side (CPU) checks of the Classify head: the builder against the reference's bookkeeping and the
module's state_dict schema (tests/golden/g13_cls.json), the plan's one classify node, launch and packed
centre tap, every refusal with its message, the detectors' ValueError, and ycx_classify's argument
validation (no device call is made)."""
import ctypes
import hashlib
import json
import os

import pytest
import torch

import cls_case as C
from helpers import sd_hash
from ycx import _lib as L
from ycx import pack
from ycx.engine import Graph, Plan, Val, check_plan_precision, lower_module
from ycx.nets.common import Classify
from ycx.nets.yolo import Model, parse_model
from ycx.schedule import Schedule
from ycx.utils.synth import synthetic_state_dict

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope='module')
def g13():
    with open(os.path.join(GOLD, 'g13_cls.json')) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def model():
    m = Model(C.cls_mini(), C.ANCHORS2, C.NC).eval()
    m.load_state_dict(synthetic_state_dict(m, seed=C.W_SEED))
    return m


def test_parse_model_builds_classify_like_the_reference(g13):
    """Fails on a tree without the feature: 'Classify' raises "out of scope" at parse time there."""
    e = g13['cls']
    layers, save = parse_model(C.cls_mini(), [3], C.ANCHORS2, C.NC)
    assert len(layers) == e['n_layers'] and save == e['save']
    assert sum(p.numel() for p in layers.parameters()) == e['n_params']
    head = layers[-1]
    assert type(head) is Classify and head.np == e['head_np'] and head.f == -1
    sd = head.state_dict()
    assert list(sd) == list(e['head_state_dict'])
    assert {k: list(v.shape) for k, v in sd.items()} == e['head_state_dict']
    assert list(sd['conv.weight'].shape) == [C.CLS_C2, C.CLS_C1, C.CLS_K, C.CLS_K] and list(sd['conv.bias'].shape) == [10]
    m = Model(C.cls_mini(), C.ANCHORS2, C.NC)
    keys = m.state_dict()
    assert len(keys) == e['n_keys']
    assert hashlib.sha256('\n'.join(sorted(keys.keys())).encode()).hexdigest() == e['keys_sha256']
    sd = synthetic_state_dict(m, seed=C.W_SEED)
    assert sd_hash(sd) == e['sd_hash']  # the fixture's weights, regenerated
    r = m.load_state_dict(sd, strict=True)
    assert not r.missing_keys and not r.unexpected_keys


def test_arguments_pass_as_written():
    """No special case in the reference's parser: c1 is explicit and not scaled by width_multiple, and the
    bookkeeping channel count after the layer is ch[f]."""
    d = C.cls_mini()
    d['width_multiple'] = 0.5  # the backbone shrinks to 16, 32, 32, 32 channels; Classify's c1 stays as written
    layers, _ = parse_model(d, [3], C.ANCHORS2, C.NC)
    assert layers[3].conv.out_channels == 32
    assert (layers[-1].conv.in_channels, layers[-1].conv.out_channels) == (C.CLS_C1, C.CLS_C2)
    d = C.cls_mini()
    d['head'].append([-1, 1, 'Conv', [32, 1, 1]])  # reads "ch[f]" = 64 channels, as the reference would build it
    layers, _ = parse_model(d, [3], C.ANCHORS2, C.NC)
    assert layers[-1].conv.in_channels == 64
    layers, _ = parse_model(C.cls_mini((64, 10, 3, 2, 1, 1)), [3], C.ANCHORS2, C.NC)
    c = layers[-1].conv
    assert (c.kernel_size, c.stride, c.padding, c.groups) == ((3, 3), (2, 2), (1, 1), 1)


def test_plan_has_one_classify_node_and_launch(model):
    plan = Plan(model, C.SHAPE)
    assert plan.counts() == {'stem': 1, 'conv': 3, 'classify': 1}  # no tonchw, no copy
    assert not plan.is_list and [(v.n, v.h, v.w, v.c, v.role) for v in plan.out_vals] == [(2, 1, 1, 10, 'output')]
    nd = plan.out_vals[0].producer
    assert nd.kind == 'classify' and nd is plan.graph.nodes[-1] and nd.out.buf is None
    x = nd.inputs[0]
    assert (x.n, x.h, x.w, x.c) == (2, 4, 4, 64)
    assert (nd.p['kernel'], nd.p['stride']) == (3, 1)
    for precision in ('f32', 'fp16', 'bf16', 'fp8'):
        check_plan_precision(plan, precision)  # an fp8 plan accepts the node
        sch = Schedule(plan, precision)
        kinds = [la.kind for la in sch.launches]
        assert kinds.count('classify') == 1 and kinds[-1] == 'classify' and 'copy' not in kinds
        assert sch.launches[-1].nodes == (nd,)
    assert plan.conv_flops == sum(pack.flops(n) for n in plan.graph.nodes)
    assert pack.flops(nd) == 2 * 2 * 10 * 64


def test_packed_weight_is_the_centre_tap_in_fp32(model):
    plan = Plan(model, C.SHAPE)
    nd = plan.graph.nodes[-1]
    conv = model.model[-1].conv
    want_w = conv.weight.detach()[:, :, 1, 1].to(torch.float32)
    assert torch.equal(nd.p['w'].reshape(10, 64), conv.weight.detach().double()[:, :, 1, 1])
    idx = pack.conv_index(plan.graph.nodes)
    assert idx[id(nd)] == 4
    for precision in ('f32', 'fp16', 'bf16', 'fp8'):
        assert pack.spec(nd, precision) == ((10, 64), torch.float32, (10,))
        wt, bt = pack.pack(nd, precision, silu_ps=False)
        assert wt.dtype == torch.float32 and tuple(wt.shape) == (10, 64) and wt.is_contiguous()
        assert torch.equal(wt, want_w) and torch.equal(bt, conv.bias.detach().to(torch.float32))
        got = pack.take_prepacked({'p8': wt, 'p9': bt}, 8, pack.spec(nd, precision))
        assert got[0] is wt and got[1] is bt
    with pytest.raises(ValueError, match='do not match this plan at tensor p8'):
        pack.take_prepacked({'p8': wt.to(torch.bfloat16), 'p9': bt}, 8, pack.spec(nd, 'bf16'))


def act(c=64, hw=4):
    return Val(2, hw, hw, c)


def test_any_stride_is_taken():
    for s in (1, 2, 3):
        g = Graph()
        out = lower_module(g, Classify(64, 10, 3, s), act())
        assert (out.n, out.h, out.w, out.c, out.role) == (2, 1, 1, 10, 'output') and g.nodes[-1].kind == 'classify'
    g = Graph()
    lower_module(g, Classify(64, 10), act())  # k = 1: the centre tap is the whole kernel
    assert tuple(g.nodes[-1].p['w'].shape) == (10, 64, 1, 1)
    g = Graph()
    lower_module(g, Classify(64, 10, 5), act())
    assert g.nodes[-1].p['kernel'] == 5


@pytest.mark.parametrize('args, values', [
    ((64, 10, 2), 'k 2, s 1, p 1, g 1'),          # even k
    ((64, 10, 4, 1, 2), 'k 4, s 1, p 2, g 1'),    # even k with p == k // 2
    ((64, 10, 3, 1, 0), 'k 3, s 1, p 0, g 1'),    # explicit other p
    ((64, 10, 3, 1, 2), 'k 3, s 1, p 2, g 1'),
    ((64, 10, 1, 1, 1), 'k 1, s 1, p 1, g 1'),
    ((64, 10, 3, 1, None, 2), 'k 3, s 1, p 1, g 2'),  # groups
])
def test_unsupported_forms_name_their_values(args, values):
    with pytest.raises(NotImplementedError, match=f'Classify with {values} has no HIP kernel'):
        lower_module(Graph(), Classify(*args), act())


def test_refusals():
    with pytest.raises(NotImplementedError, match='Classify reads one layer'):
        parse_model(C.cls_mini(frm=[-1, -2]), [3], C.ANCHORS2, C.NC)
    with pytest.raises(NotImplementedError, match='Classify reads one layer'):
        lower_module(Graph(), Classify(64, 10), [act(), act()])
    with pytest.raises(NotImplementedError, match='Classify on the model input'):
        lower_module(Graph(), Classify(3, 10), Val(2, 64, 64, 3, role='input'))
    d = {'depth_multiple': 1.0, 'width_multiple': 1.0, 'backbone': [[-1, 1, 'Classify', [3, 10]]], 'head': []}
    with pytest.raises(NotImplementedError, match='Classify on the model input'):
        Plan(Model(d, C.ANCHORS2, C.NC).eval(), C.SHAPE)
    for c in (4, 12, 60):
        with pytest.raises(NotImplementedError, match=f'Classify on {c} channels has no HIP kernel: ycx_classify takes '
                                                      f'a channel slice that is a multiple of 8'):
            lower_module(Graph(), Classify(c, 10), act(c))
    with pytest.raises(ValueError, match='Classify built for 32 input channels reads a layer of 64'):
        lower_module(Graph(), Classify(32, 10), act())


def test_classify_anywhere_but_last_is_refused():
    d = C.cls_mini()
    d['head'].append([-2, 1, 'Conv', [32, 1, 1]])  # a layer after the head, reading layer 3
    with pytest.raises(NotImplementedError, match="Classify is lowered only as the model's last layer"):
        Plan(Model(d, C.ANCHORS2, C.NC).eval(), C.SHAPE)
    d = C.cls_mini()
    d['head'].append([-1, 1, 'nn.Upsample', ['None', 2, 'nearest']])  # a layer reading the logits
    with pytest.raises(NotImplementedError, match="Classify is lowered only as the model's last layer"):
        Plan(Model(d, C.ANCHORS2, C.NC).eval(), C.SHAPE)


@pytest.mark.parametrize('name', ['Shortcut', 'Stem', 'GhostStem', 'Chuncat', 'Foldcut', 'TransformerBlock',
                                  'RepBottleneckCSPA'])
def test_still_out_of_scope(name):
    d = {'depth_multiple': 1.0, 'width_multiple': 1.0, 'backbone': [[-1, 1, name, [64]]], 'head': []}
    with pytest.raises(NotImplementedError, match='out of scope'):
        parse_model(d, [3], C.ANCHORS2, C.NC)


def test_detectors_refuse_a_classify_model(model):
    from ycx.detect import ConcurrentDetector, Detector, PipelinedDetector
    mask = [[3, 4, 5], [0, 1, 2]]
    for cls in (Detector, PipelinedDetector, ConcurrentDetector):
        with pytest.raises(ValueError, match='Classify head'):
            cls(model, C.SHAPE, 'cuda', C.ANCHORS2, mask)


def test_predict_refuses_a_classify_model(model):
    from ycx.detect import _require_detect_head
    with pytest.raises(ValueError, match='no boxes to decode'):
        _require_detect_head(model)
    _require_detect_head(Model('yolov7-tiny', C.ANCHORS2 + [[1, 2, 3, 4, 5, 6]], C.NC))


def desc(**kw):
    d = L.ClassifyDesc()
    d.n, d.h, d.w, d.c, d.in_c_off, d.in_c_stride, d.cout, d.dtype, d.dequant = 2, 4, 4, 64, 8, 80, 10, L.DT_BF16, 1.0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def call(d, x=1 << 20, w=1 << 20, bias=1 << 20, y=1 << 20, ws=1 << 20):
    """Non-null, never dereferenced pointers: every case below must return before any device call."""
    return L.lib.ycx_classify(ctypes.byref(d) if d is not None else None, x, w, bias, y, ws, None)


def test_bad_arguments_without_a_device():
    assert ctypes.sizeof(L.ClassifyDesc) == 36 < 2 * ctypes.sizeof(L.ConvDesc)
    assert ctypes.sizeof(L.Op) == L.lib.ycx_struct_size(8) and L.OP_CLASSIFY == 13 and L.ABI_VERSION == 9
    assert call(None) == L.YCX_ERR_BAD_ARG
    for null in ('x', 'w', 'y', 'ws'):
        assert call(desc(), **{null: None}) == L.YCX_ERR_BAD_ARG, null
    bad = [dict(dtype=4), dict(dtype=-1), dict(c=60, in_c_stride=76), dict(in_c_off=4), dict(in_c_stride=84),
           dict(in_c_off=24), dict(in_c_off=-8), dict(n=0), dict(h=0), dict(w=-1), dict(c=0), dict(cout=0),
           dict(in_c_stride=0)]
    for kw in bad:
        assert call(desc(**kw)) == L.YCX_ERR_BAD_ARG, kw
    op = L.Op()
    op.kind = L.OP_CLASSIFY
    op.d.classify = desc()
    assert L.lib.ycx_run_ops(ctypes.byref(op), 1, None, None) == L.YCX_ERR_BAD_ARG  # null pointers, through the executor
