"""Grouped and depthwise convs end to end: the gx-mini config (tests/grouped_case.py: dw_conv, ResX,
ResXCSPC, ResCSPA, Bottleneck g = 4, RobustConv, a grouped conv into a concat slice and one under an
upsample, two-level IDetect) through Model.forward against the reference's own eval outputs
(tests/golden/g6_grouped.npz, made by tests/golden/make_golden_grouped.py).

Bars, max |gpu - ref| / max |ref| per output tensor: TOL of tests/test_gpu_p6.py (f32 1e-3, fp16 1e-3,
bf16 2.5e-2), the bars G2, G4 and G5 are held to."""
import json
import os

import numpy as np
import pytest
import torch

import grouped_case as C
from helpers import rel_err, sd_hash
from test_gpu_p6 import TOL
from ycx import _lib as L
from ycx.nets.yolo import Model
from ycx.utils.synth import synthetic_images, synthetic_state_dict

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope='module')
def g6():
    with open(os.path.join(GOLD, 'g6_grouped.json')) as f:
        meta = json.load(f)
    return meta['gx_mini'], dict(np.load(os.path.join(GOLD, 'g6_grouped.npz')))


def gx_model(precision, meta):
    m = Model(C.gx_mini(), C.ANCHORS2, C.NC, precision=precision).eval()
    sd = synthetic_state_dict(m, seed=C.W_SEED)
    assert sd_hash(sd) == meta['sd_hash']  # the fixture's weights, regenerated
    m.load_state_dict(sd)
    return m


@pytest.mark.parametrize('precision', ['f32', 'fp16', 'bf16'])
def test_gx_mini_vs_reference(device, g6, precision):
    meta, gold = g6
    m = gx_model(precision, meta).to(device)
    x = synthetic_images(*C.SHAPE, seed=C.IMG_SEED).to(device)
    z, xs = m(x)
    assert len(xs) == 2 and [C.SHAPE[2] / t.shape[2] for t in xs] == C.STRIDES
    errs = {'z': rel_err(z.cpu(), torch.from_numpy(gold['z']))}
    for j, t in enumerate(xs):
        g = torch.from_numpy(gold[f'x{j}'])
        assert tuple(t.shape) == tuple(g.shape)
        errs[f'x{j}'] = rel_err(t.cpu(), g)
    print(f"\n{precision} G6 gx-mini rel err {errs}")
    assert max(errs.values()) < TOL[precision], errs
    eng = m.engine_for(x.shape, device, slot=m.EAGER_SLOT)
    kinds = [i['kind'] for i in eng.op_info]
    assert kinds.count('gconv') == C.N_GCONV
    # the only copy kernel is the upsample under the grouped conv; no concat slice is copied
    assert [i['name'] for i in eng.op_info if i['kind'] == 'copy'] == ['upsample2x']
    assert sum(1 for i in range(eng.n_ops) if eng.ops[i].kind == L.OP_GCONV) == C.N_GCONV
    for i in range(eng.n_ops):  # plain SiLU, fp32 weights, in every precision
        if eng.ops[i].kind == L.OP_GCONV:
            assert eng.ops[i].d.conv.act == L.ACT_SILU and eng.ops[i].d.conv.groups > 1


@pytest.mark.parametrize('precision', ['bf16', 'fp16'])
def test_gx_graph_replay_matches_eager(device, g6, precision):
    meta, _ = g6
    m = gx_model(precision, meta).to(device)
    x = synthetic_images(*C.SHAPE, seed=C.IMG_SEED).to(device)
    eng = m.engine_for(x.shape, device)
    eager = [o.clone() for o in eng.run(x)]
    eng.bind_static(x)
    eng.capture()
    first = [o.clone() for o in eng.replay()]
    torch.cuda.synchronize()
    second = eng.replay()
    torch.cuda.synchronize()
    for a, b, c in zip(eager, first, second):
        assert torch.equal(a, b) and torch.equal(b, c)


def test_gx_prepack_roundtrip(device, g6, tmp_path):
    """Grouped weights go through the prepack file as fp32 [kh][kw][cout][cin_g]: saved, loaded into a
    freshly initialised module, the forward is bit-identical."""
    meta, _ = g6
    m = gx_model('bf16', meta).to(device)
    x = synthetic_images(*C.SHAPE, seed=C.IMG_SEED).to(device)
    ref = [o.clone() for o in m.engine_for(x.shape, device).run(x)]
    path = str(tmp_path / 'gx.safetensors')
    m.save_prepacked(path, C.SHAPE[2:], device=device)
    eng = m.engine_for(x.shape, device)
    gi = next(i for i, nd in enumerate(nd for nd in eng.graph.nodes if nd.kind in ('conv', 'stem', 'stem_reorg', 'gconv'))
              if nd.kind == 'gconv')
    assert eng.packed[f'p{2 * gi}'].dtype == torch.float32 and tuple(eng.packed[f'p{2 * gi}'].shape) == (3, 3, 64, 1)
    m2 = Model(C.gx_mini(), C.ANCHORS2, C.NC, precision='bf16').eval().to(device)  # random weights
    m2.load_prepacked(path)
    for a, b in zip(ref, m2.engine_for(x.shape, device).run(x)):
        assert torch.equal(a, b)


@pytest.mark.parametrize('precision', ['bf16', 'f32'])
def test_gx_chunked_ops_bit_identical(device, g6, precision, monkeypatch):
    """YCX_CHUNK over the whole plan (one image at a time): the grouped ops are image-major like the
    rest, so the chunked run equals the unchunked one bit for bit."""
    meta, _ = g6
    m = gx_model(precision, meta).to(device)
    x = synthetic_images(*C.SHAPE, seed=C.IMG_SEED).to(device)
    eng = m.engine_for(x.shape, device)
    eng.bind_static(x)
    whole = [o.clone() for o in eng.run_static()]
    monkeypatch.setenv('YCX_CHUNK', f'1:{eng.n_ops}')
    ops, n_ops = eng._exec_ops()
    assert n_ops == 2 * eng.n_ops and sum(1 for i in range(n_ops) if ops[i].kind == L.OP_GCONV) == 2 * C.N_GCONV
    for a, b in zip(whole, eng.run_static()):
        assert torch.equal(a, b)


def test_gx_fp8_is_refused(device, g6):
    meta, _ = g6
    m = gx_model('fp8', meta).to(device)
    x = synthetic_images(*C.SHAPE, seed=C.IMG_SEED).to(device)
    with pytest.raises(NotImplementedError, match='grouped conv has no fp8 path'):
        m(x)
