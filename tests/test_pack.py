"""Host-side (CPU) checks of ycx.pack and of what Engine binds from it: for every case of tests/pack_case.py
the ops, descriptors, op_info and packed bytes of an Engine built on CPU memory against
tests/golden/g10_pack.json, which was recorded from the packers and hand-filled descriptors Engine carried
before packing was a module of its own (the file's "parent" commit; tests/golden/make_golden_pack.py);
and ``pack.pack`` / ``pack.spec`` / ``pack.desc`` / ``pack.flops`` / ``pack.take_prepacked`` on their own."""
import json
import os

import pytest
import torch

import pack_case as C
from ycx import _lib as L
from ycx import engine, pack

CASES = C.cases()
SKIPPED_FIELDS = ('tile', 'k_split')  # Engine sets them after pack.desc


@pytest.fixture(scope='module')
def golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g10_pack.json')) as f:
        g = json.load(f)
    assert len(g['parent']) == 40 and list(g['cases']) == list(CASES)
    assert len({json.dumps(row) for row in g['table']}) == len(g['table'])
    return {name: C.expand(case, g['table']) for name, case in g['cases'].items()}


@pytest.fixture(scope='module', params=list(CASES))
def built(request):
    """(case id, plan, precision, CPU engine), with engine._NO_SILU_PS as the case says for as long as the
    case's tests run (module scope: pytest runs a case's tests together, one engine alive at a time)."""
    net, shape, precision, no_silu_ps = CASES[request.param]
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(engine, '_NO_SILU_PS', no_silu_ps)
        plan = C.plan(net, shape)
        yield request.param, plan, precision, C.cpu_engine(plan, precision)


def test_engine_matches_the_recorded_one(built, golden):
    name, _, _, e = built
    got, want = json.loads(json.dumps(C.encode(e))), golden[name]
    assert list(got) == list(want)
    for key in want:
        if key in ('ops', 'packed'):
            assert len(got[key]) == len(want[key]), key
            for i, (g, w) in enumerate(zip(got[key], want[key])):
                assert g == w, f"{name}: {key}[{i}]"
        else:
            assert got[key] == want[key], key


def test_engine_bound_to_its_own_prepacked_tensors_is_the_same(built, golden):
    name, plan, precision, e = built
    again = C.cpu_engine(plan, precision, prepacked=dict(e.packed))
    assert json.loads(json.dumps(C.encode(again))) == golden[name]


def node_descs(e):
    """[(node, its descriptor in the op array, bf16_weights, pool)] over the engine's launches."""
    out = []
    assert len(e.schedule.launches) == e.n_ops
    for i, la in enumerate(e.schedule.launches):
        op, nd = e.ops[i], la.nodes
        if la.kind == 'stem2':
            out += [(nd[0], op.d.pair[0], False, None), (nd[1], op.d.pair[1], True, None)]
        elif la.kind == 'conv_pair':
            out += [(nd[0], op.d.pair[0], False, None), (nd[1], op.d.pair[1], False, None)]
            if len(nd) > 2:
                out.append((nd[2], op.conv3, False, nd[3]))
        elif la.kind == 'conv':
            out.append((nd[0], op.d.conv, False, nd[1] if len(nd) > 1 else None))
        elif la.kind in ('gconv', 'deconv', 'ghost'):
            out.append((nd[0], op.d.conv, False, None))
    return out


def test_pack_alone_gives_the_recorded_tensors_and_descriptors(built, golden):
    """Without an Engine: pack.pack has the shape and dtype pack.spec says and the fixture's bytes, pack.desc
    every descriptor field Engine does not set afterwards, pack.flops the plan's and the engine's FLOPs."""
    name, plan, precision, e = built
    recorded = {row[0]: row[1:] for row in golden[name]['packed']}
    index = pack.conv_index(plan.graph.nodes)
    convs = node_descs(e)
    assert sorted(index[id(nd)] for nd, *_ in convs) == list(range(len(index))) and 2 * len(index) == len(recorded)
    for nd, d, bf16_weights, pool in convs:
        silu_ps = (nd.kind in pack.DENSE and nd.p['act'] == L.ACT_SILU and precision != 'f32'
                   and not engine._NO_SILU_PS)
        wshape, wdt, bshape = pack.spec(nd, precision, bf16_weights)
        wt, bt = pack.pack(nd, precision, bf16_weights=bf16_weights, silu_ps=silu_ps,
                           in_scale=pack.scale_of(e.scales, nd.inputs[0]))
        i = 2 * index[id(nd)]
        assert (tuple(wt.shape), wt.dtype, tuple(bt.shape), bt.dtype) == (wshape, wdt, bshape, torch.float32)
        assert wt.device.type == bt.device.type == 'cpu'
        assert recorded[f"p{i}"] == [list(wshape), str(wdt), C.tensor_hash(wt)], f"{name}: p{i} ({nd.kind})"
        assert recorded[f"p{i + 1}"] == [list(bshape), 'torch.float32', C.tensor_hash(bt)], f"{name}: p{i + 1}"
        took = pack.take_prepacked(e.packed, i, (wshape, wdt, bshape))  # the case's own tensors
        assert took[0] is e.packed[f"p{i}"] and took[1] is e.packed[f"p{i + 1}"]
        got = pack.desc(nd, precision, bf16_weights=bf16_weights, silu_ps=silu_ps, scales=e.scales, pool=pool)
        assert got.tile == 0 and got.k_split == 0
        for field, _ in L.ConvDesc._fields_:
            if field not in SKIPPED_FIELDS:
                assert getattr(got, field) == getattr(d, field), f"{name}: {nd.kind} p{i} {field}"
    total = sum(pack.flops(nd) for nd in plan.graph.nodes if nd.kind in pack.CONV_KINDS)
    assert total == plan.conv_flops == e.conv_flops == golden[name]['conv_flops']


@pytest.mark.gpu
def test_engine_on_the_device_holds_what_pack_packs(device):
    from helpers import make_model
    e = engine.Engine(make_model('yolov7-tiny', 1, 0)[0], (1, 3, 160, 160), device, 'bf16')
    index = pack.conv_index(e.graph.nodes)
    convs = node_descs(e)
    assert len(convs) == len(index) and len(e.packed) == 2 * len(index)
    for nd, _, bf16_weights, _ in convs:
        silu_ps = nd.kind in pack.DENSE and nd.p['act'] == L.ACT_SILU and not engine._NO_SILU_PS
        wt, bt = pack.pack(nd, 'bf16', bf16_weights=bf16_weights, silu_ps=silu_ps)
        i = 2 * index[id(nd)]
        for t, name in ((wt, f"p{i}"), (bt, f"p{i + 1}")):
            on_device = e.packed[name]
            assert on_device.device.type == 'cuda' and (on_device.shape, on_device.dtype) == (t.shape, t.dtype)
            assert C.tensor_hash(on_device) == C.tensor_hash(t), name
    e.close()


# one node of each conv kind, on the small networks
KIND_NET = {'conv': 'gx-mini', 'stem': 'gx-mini', 'gconv': 'gx-mini', 'stem_reorg': 'p6-mini', 'deconv': 'rc2-mini',
            'ghost': 'gh-mini'}


@pytest.mark.parametrize('precision', ['bf16', 'f32'])
@pytest.mark.parametrize('kind', list(KIND_NET))
def test_take_prepacked_refuses_what_does_not_match(kind, precision):
    assert set(KIND_NET) == set(pack.CONV_KINDS)
    net = KIND_NET[kind]
    plan = C.plan(net, next(shape for n, shape, _ in C.SHAPES if n == net))
    nd = next(nd for nd in plan.graph.nodes if nd.kind == kind)
    i = 2 * pack.conv_index(plan.graph.nodes)[id(nd)]
    spec = pack.spec(nd, precision)
    wt, bt = pack.pack(nd, precision, silu_ps=False)
    own = {f"p{i}": wt, f"p{i + 1}": bt, "p9999": wt}
    got = pack.take_prepacked(own, i, spec)
    assert got[0] is wt and got[1] is bt
    other = torch.float16 if wt.dtype != torch.float16 else torch.bfloat16
    bad = {'no weight': {f"p{i + 1}": bt}, 'no bias': {f"p{i}": wt},
           'weight shape': dict(own, **{f"p{i}": wt.reshape(-1)}),
           'weight shape, same numel': dict(own, **{f"p{i}": wt.transpose(0, -1)}) if wt.shape[0] != wt.shape[-1]
           else dict(own, **{f"p{i}": wt[:-1]}),
           'weight dtype': dict(own, **{f"p{i}": wt.to(other)}),
           'bias shape': dict(own, **{f"p{i + 1}": bt[:-1]}),
           'bias dtype': dict(own, **{f"p{i + 1}": bt.to(torch.float64)}),
           'bias in bf16': dict(own, **{f"p{i + 1}": bt.to(torch.bfloat16)})}
    for what, tensors in bad.items():
        with pytest.raises(ValueError, match=rf"prepacked weights do not match this plan at tensor p{i}$"):
            pack.take_prepacked(tensors, i, spec)
