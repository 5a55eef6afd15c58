"""The Classify head and the Rep blocks end to end: tests/cls_case.py's cls-mini (four Convs to a 4 x 4 x 64
map, Classify [64, 10, 3]) and rep-mini (RepBottleneck, RepRes, RepResX, RepResCSPA, RepResXCSPC) through
Model.forward against the reference's own eval outputs (tests/golden/g13_cls.npz, made by
tests/golden/make_golden_cls.py), as max |gpu - ref| / max |ref| under TOL of tests/test_gpu_p6.py (f32 1e-3,
fp16 1e-3, bf16 2.5e-2, fp8 0.12). The same logits must come back eagerly, from a captured graph and after a
save_prepacked / load_prepacked round trip."""
import json
import os

import numpy as np
import pytest
import torch

import cls_case as C
from helpers import rel_err, sd_hash
from test_gpu_p6 import TOL
from ycx import _lib as L
from ycx.nets.yolo import Model
from ycx.utils.synth import synthetic_images, synthetic_state_dict

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope='module')
def g13():
    with open(os.path.join(GOLD, 'g13_cls.json')) as f:
        meta = json.load(f)
    return meta, dict(np.load(os.path.join(GOLD, 'g13_cls.npz')))


def make(cfg, precision, meta=None):
    m = Model(cfg, C.ANCHORS2, C.NC, precision=precision).eval()
    sd = synthetic_state_dict(m, seed=C.W_SEED)
    if meta is not None:
        assert sd_hash(sd) == meta['sd_hash']  # the fixture's weights, regenerated
    m.load_state_dict(sd)
    return m


def image(device):
    return synthetic_images(*C.SHAPE, seed=C.IMG_SEED).to(device)


@pytest.mark.parametrize('precision', ['f32', 'fp16', 'bf16', 'fp8'])
def test_cls_mini_vs_reference(device, g13, precision):
    meta, gold = g13
    m = make(C.cls_mini(), precision, meta['cls']).to(device)
    x = image(device)
    y = m(x)
    assert torch.is_tensor(y) and tuple(y.shape) == (2, 10) == tuple(meta['cls']['out_shape'])
    assert y.dtype == torch.float32 and y.is_contiguous()
    err = rel_err(y.cpu(), torch.from_numpy(gold['cls']))
    print(f"\n{precision} G13 cls-mini logits rel err {err:.3e}")
    assert err < TOL[precision], err
    eng = m.engine_for(x.shape, device, slot=m.EAGER_SLOT)
    assert [i['kind'] for i in eng.op_info].count('classify') == 1 and eng.op_info[-1]['kind'] == 'classify'
    assert eng.ops[eng.n_ops - 1].kind == L.OP_CLASSIFY and 'copy' not in [i['kind'] for i in eng.op_info]
    assert len(eng.scratch) == 1 and tuple(eng.scratch[0].shape) == (2, 64) and eng.scratch[0].dtype == torch.float32
    wt = eng.packed['p8']
    assert wt.dtype == torch.float32 and tuple(wt.shape) == (10, 64)
    assert torch.equal(wt.cpu(), m.model[-1].conv.weight.detach().cpu()[:, :, 1, 1])
    if precision == 'fp8':
        assert all(t.dtype == torch.float8_e4m3fn for t in eng.buffers)
        d = eng.ops[eng.n_ops - 1].d.classify
        assert d.dequant == 1.0 / eng.scales[id(eng.graph.nodes[-1].inputs[0].buf)] and d.dtype == L.DT_FP8
    # the workspace holds the means of the last activation
    last = eng.graph.nodes[-1].inputs[0].buf.tensor
    if precision != 'fp8':
        assert rel_err(eng.scratch[0].cpu(), last.float().mean((1, 2)).cpu()) < 1e-6


@pytest.mark.parametrize('precision', ['f32', 'fp16', 'bf16', 'fp8'])
def test_cls_graph_replay_matches_eager(device, g13, precision):
    meta, _ = g13
    m = make(C.cls_mini(), precision, meta['cls']).to(device)
    x = image(device)
    eng = m.engine_for(x.shape, device)
    eager = eng.run(x).clone()
    eng.bind_static(x)
    eng.capture()
    first = eng.replay().clone()
    torch.cuda.synchronize()
    second = eng.replay()
    torch.cuda.synchronize()
    assert tuple(eager.shape) == (2, 10) and torch.equal(eager, first) and torch.equal(first, second)
    assert torch.equal(eager, m(x))


@pytest.mark.parametrize('precision', ['f32', 'fp16', 'bf16', 'fp8'])
def test_cls_prepack_roundtrip(device, g13, tmp_path, precision):
    """The centre tap and the bias travel as tensors p8 / p9: saved and loaded into a freshly initialised
    module, the logits are bit-identical."""
    meta, _ = g13
    m = make(C.cls_mini(), precision, meta['cls']).to(device)
    x = image(device)
    ref = m(x).clone()
    path = str(tmp_path / 'cls.safetensors')
    info = m.save_prepacked(path, C.SHAPE[2:], device=device)
    assert info['n_tensors'] == 10
    m2 = Model(C.cls_mini(), C.ANCHORS2, C.NC, precision='bf16' if precision == 'f32' else 'f32').eval().to(device)  # random weights, another precision
    m2.load_prepacked(path)
    assert m2.precision == precision
    y2 = m2(x)
    assert tuple(y2.shape) == (2, 10) and torch.equal(ref, y2)


def test_fp16_range_guard_sees_the_logits(device, g13):
    """An activation past the fp16 range reaches the logits as inf / NaN: the forward warns, re-plans in bf16
    and still returns [2, 10]."""
    meta, _ = g13
    m = make(C.cls_mini(), 'fp16', meta['cls'])
    with torch.no_grad():
        m.model[0].bn.weight.mul_(1e6)
    m.invalidate(weights_changed=True)
    m.to(device)
    with pytest.warns(RuntimeWarning, match='fp16 plan overflowed'):
        y = m(image(device))
    assert m.precision == 'bf16' and tuple(y.shape) == (2, 10) and y.dtype == torch.float32


@pytest.mark.parametrize('precision', ['f32', 'fp16', 'bf16'])
def test_rep_mini_vs_reference(device, g13, precision):
    meta, gold = g13
    m = make(C.rep_mini(), precision, meta['rep']).to(device)
    x = image(device)
    y = m(x)
    assert tuple(y.shape) == C.REP_OUT == tuple(meta['rep']['out_shape']) and y.dtype == torch.float32
    err = rel_err(y.cpu(), torch.from_numpy(gold['rep']))
    print(f"\n{precision} G13 rep-mini rel err {err:.3e}")
    assert err < TOL[precision], err
    eng = m.engine_for(x.shape, device, slot=m.EAGER_SLOT)
    assert [i['kind'] for i in eng.op_info].count('gconv') == 2
    eng2 = m.engine_for(x.shape, device)
    eng2.bind_static(x)
    eng2.capture()
    assert torch.equal(eng2.replay(), y)
    torch.cuda.synchronize()


def test_rep_mini_has_no_fp8_plan(device, g13):
    meta, _ = g13
    m = make(C.rep_mini(), 'fp8', meta['rep']).to(device)
    with pytest.raises(NotImplementedError, match='grouped conv has no fp8 path'):
        m(image(device))
