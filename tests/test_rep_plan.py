"""Host-side (CPU) checks of the Rep blocks (RepBottleneck, RepRes, RepResX, RepResCSPA/B/C, RepResXCSPA/B/C):
the builder against the reference's bookkeeping (tests/golden/g13_cls.json), each RepConv lowered to one
conv / gconv node whose folded weights equal the reference's get_equivalent_kernel_bias restated in float64,
the reference's RepBottleneck quirk, the grouped limits and the fp8 refusal, and the names that stay out of
scope."""
import hashlib
import json
import os

import pytest
import torch
from torch import nn

import cls_case as C
from helpers import sd_hash
from ycx import _lib as L
from ycx.engine import Plan, check_plan_precision
from ycx.nets import common as N
from ycx.nets.yolo import _CONV_LIKE, _CSP_LIKE, Model, parse_model
from ycx.schedule import Schedule
from ycx.utils.synth import synthetic_state_dict

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope='module')
def g13():
    with open(os.path.join(GOLD, 'g13_cls.json')) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def model():
    m = Model(C.rep_mini(), C.ANCHORS2, C.NC).eval()
    m.load_state_dict(synthetic_state_dict(m, seed=C.W_SEED))
    return m


def keys_hash(sd):
    return hashlib.sha256('\n'.join(sorted(sd.keys())).encode()).hexdigest()


def test_parse_model_builds_rep_mini_like_the_reference(g13):
    """Fails on a tree without the feature: 'RepBottleneck' raises "out of scope" at parse time there."""
    e = g13['rep']
    layers, save = parse_model(C.rep_mini(), [3], C.ANCHORS2, C.NC)
    assert len(layers) == e['n_layers'] and save == e['save']
    assert sum(p.numel() for p in layers.parameters()) == e['n_params']
    assert [type(m).__name__ for m in layers] == ['Conv', 'Conv', 'RepBottleneck', 'RepRes', 'Conv', 'RepResX',
                                                  'RepResCSPA', 'RepResXCSPC', 'Conv']
    m = Model(C.rep_mini(), C.ANCHORS2, C.NC)
    assert len(m.state_dict()) == e['n_keys'] and keys_hash(m.state_dict()) == e['keys_sha256']
    sd = synthetic_state_dict(m, seed=C.W_SEED)
    assert sd_hash(sd) == e['sd_hash']  # the fixture's weights, regenerated
    r = m.load_state_dict(sd, strict=True)
    assert not r.missing_keys and not r.unexpected_keys


@pytest.mark.parametrize('name', sorted(C.SINGLES))
def test_every_rep_block_builds_like_the_reference(g13, name):
    e = g13['singles'][name]
    module, args, c_in = C.SINGLES[name]
    m = Model(C.single(module, args, c_in), C.ANCHORS2, C.NC)
    assert len(m.model) == e['n_layers'] and m.save == e['save']
    assert sum(p.numel() for p in m.parameters()) == e['n_params']
    assert len(m.state_dict()) == e['n_keys'] and keys_hash(m.state_dict()) == e['keys_sha256']
    assert list(m.model[-1].state_dict()) == e['block_keys']  # the block's own keys, in the reference's order
    cls = getattr(N, name)
    assert type(m.model[-1]) is cls and cls in _CONV_LIKE
    assert (cls in _CSP_LIKE) == ('CSP' in name)
    Plan(m.eval(), C.SHAPE)  # and it lowers


def test_constructors_keep_the_reference_defaults():
    import inspect
    d = {n: inspect.signature(getattr(N, n).__init__).parameters for n in C.SINGLES}
    assert [d[n]['g'].default for n in sorted(d)] == [1, 1, 1, 1, 1, 32, 32, 32, 32]
    assert {n: d[n]['shortcut'].default for n in d if 'CSPB' in n} == {'RepResCSPB': False, 'RepResXCSPB': False}
    assert all(d[n]['shortcut'].default is True for n in d if 'CSPB' not in n)
    # the inner blocks: RepRes / RepResX with e = 0.5 in every CSP form
    for name, hidden in (('RepResCSPA', 64), ('RepResCSPB', 128), ('RepResCSPC', 64), ('RepResXCSPA', 64),
                         ('RepResXCSPB', 128), ('RepResXCSPC', 64)):
        b = getattr(N, name)(128, 128, 2)
        assert len(b.m) == 2
        for inner in b.m:
            assert type(inner) is (N.RepResX if 'X' in name else N.RepRes)
            rc = inner.cv2
            assert type(rc) is N.RepConv and rc.in_channels == rc.out_channels == hidden // 2
            assert rc.groups == (32 if 'X' in name else 1) and rc.rbr_identity is not None


def test_repbottleneck_keeps_the_reference_quirk():
    """The parent is built with shortcut=True, g=1, e=0.5 whatever was given; the RepConv from the e given."""
    b = N.RepBottleneck(64, 64, False, 4, 0.5)
    assert b.add is True and b.cv1.conv.out_channels == 32
    assert (b.cv2.in_channels, b.cv2.out_channels, b.cv2.groups) == (32, 64, 4) and b.cv2.rbr_identity is None
    assert list(b.state_dict())[:6] == ['cv1.conv.weight', 'cv1.bn.weight', 'cv1.bn.bias', 'cv1.bn.running_mean',
                                        'cv1.bn.running_var', 'cv1.bn.num_batches_tracked']
    # e = 1.0, what RepBottleneckCSPA/B/C pass: cv1 emits 32 channels into a RepConv sized for 64, which fails in
    # the reference's own forward and here at lowering
    q = N.RepBottleneck(64, 64, True, 1, 1.0)
    assert q.cv1.conv.out_channels == 32 and q.cv2.in_channels == 64
    d = C.single('RepBottleneck', [64, True, 1, 1.0])
    with pytest.raises(NotImplementedError, match='mismatched conv'):
        Plan(Model(d, C.ANCHORS2, C.NC).eval(), C.SHAPE)


@pytest.mark.parametrize('name', ['RepBottleneckCSPA', 'RepBottleneckCSPB', 'RepBottleneckCSPC', 'Shortcut', 'Stem',
                                  'GhostStem', 'Chuncat', 'Foldcut', 'TransformerBlock'])
def test_still_out_of_scope(name):
    d = {'depth_multiple': 1.0, 'width_multiple': 1.0, 'backbone': [[-1, 1, name, [64]]], 'head': []}
    with pytest.raises(NotImplementedError, match='out of scope'):
        parse_model(d, [3], C.ANCHORS2, C.NC)


def equivalent_kernel_bias(rc):
    """get_equivalent_kernel_bias / _fuse_bn_tensor (the reference's nets/common.py:488-529) restated in float64."""
    def fuse(w, bn):
        std = (bn.running_var.double() + bn.eps).sqrt()
        t = (bn.weight.detach().double() / std).reshape(-1, 1, 1, 1)
        return w * t, bn.bias.detach().double() - bn.running_mean.double() * bn.weight.detach().double() / std

    k3, b3 = fuse(rc.rbr_dense[0].weight.detach().double(), rc.rbr_dense[1])
    k1, b1 = fuse(rc.rbr_1x1[0].weight.detach().double(), rc.rbr_1x1[1])
    k, b = k3 + nn.functional.pad(k1, [1, 1, 1, 1]), b3 + b1
    if rc.rbr_identity is not None:
        dim = rc.in_channels // rc.groups
        idk = torch.zeros(rc.in_channels, dim, 3, 3, dtype=torch.float64)
        for i in range(rc.in_channels):
            idk[i, i % dim, 1, 1] = 1
        kid, bid = fuse(idk, rc.rbr_identity)
        k, b = k + kid, b + bid
    return k, b


def test_each_repconv_is_one_folded_node(model):
    plan = Plan(model, C.SHAPE)
    counts = plan.counts()
    assert counts['gconv'] == 2 and counts['stem'] == 1 and 'classify' not in counts
    assert [nd.kind for nd in plan.graph.nodes if nd.kind == 'tonchw'] == ['tonchw']
    assert [(v.n, v.c, v.h, v.w) for v in plan.out_vals] == [C.REP_OUT]
    mods = dict(model.model.named_modules())
    nodes3 = [nd for nd in plan.graph.nodes if nd.kind in ('conv', 'gconv') and nd.p['k'] == 3]
    found = 0
    for path, groups, kind in C.REP_CONVS:
        rc = mods[path]
        assert type(rc) is N.RepConv and rc.groups == groups
        k, b = equivalent_kernel_bias(rc)
        match = [nd for nd in nodes3 if nd.p['w'].shape == k.shape and torch.equal(nd.p['w'], k)]
        assert len(match) == 1, path
        nd = match[0]
        # the bias: the reference divides mean * gamma by std, fold_bn multiplies mean by gamma / std (one float64 ulp)
        assert nd.kind == kind and nd.p['w'].dtype == torch.float64
        assert torch.allclose(nd.p['b'], b, rtol=0, atol=1e-15)
        assert (nd.p['s'], nd.p['p'], nd.p['act']) == (1, 1, L.ACT_SILU)
        assert nd.p.get('groups', 1) == groups and int(k.shape[1]) * groups == rc.in_channels
        found += 1
    assert found == 5
    # RepBottleneck's shortcut is its RepConv's epilogue residual; RepRes / RepResX add theirs in cv3
    rb = [nd for nd in nodes3 if nd.p['residual'] is not None]
    assert len(rb) == 1 and tuple(rb[0].p['w'].shape) == (64, 32, 3, 3) and rb[0].p['residual'].c == 64
    assert [int(nd.p['w'].shape[1]) for nd in plan.graph.nodes if nd.kind == 'gconv'] == [4, 2]  # cin_g
    for precision in ('f32', 'fp16', 'bf16'):
        check_plan_precision(plan, precision)
        kinds = [la.kind for la in Schedule(plan, precision).launches]
        assert kinds.count('gconv') == 2
    with pytest.raises(NotImplementedError, match='grouped conv has no fp8 path'):
        check_plan_precision(plan, 'fp8')


def test_deployed_repconv_in_a_rep_block(model):
    """A RepRes whose RepConv was re-parameterised (rbr_reparam) lowers to the same node."""
    blk = N.RepRes(64, 64)
    blk.cv2 = N.RepConv(32, 32, 3, 1, g=1, deploy=True)
    from ycx.engine import Graph, Val, lower_module
    g = Graph()
    lower_module(g, blk.eval(), Val(2, 8, 8, 64))
    nd = g.nodes[1]
    assert nd.kind == 'conv' and torch.equal(nd.p['w'], blk.cv2.rbr_reparam.weight.detach().double())


def test_grouped_limits_raise_as_grouped_convs_do():
    # RepResX's default g = 32 on 64 channels: c_ = 32, cin_g 1 is taken; on 96 hidden channels cin_g 3 is not
    d = C.single('RepResX', [192], 128)
    with pytest.raises(NotImplementedError, match='grouped conv with cin_g 3'):
        Plan(Model(d, C.ANCHORS2, C.NC).eval(), C.SHAPE)
    d = C.single('RepResX', [128, True, 2], 128)  # cin_g 32
    with pytest.raises(NotImplementedError, match='grouped conv with cin_g 32'):
        Plan(Model(d, C.ANCHORS2, C.NC).eval(), C.SHAPE)
