"""The Ghost family end to end: the gh-mini config (tests/ghost_case.py: GhostConv k1 / s1 and k3 / s2, Ghost
s1 and s2, GhostCSPA / B / C, GhostSPPCSPC, a Ghost output in a concat slice and a GhostConv output under an
upsample, two-level IDetect) through Model.forward against the reference's own eval outputs
(tests/golden/g9_ghost.npz, made by tests/golden/make_golden_ghost.py).

Bars, max |gpu - ref| / max |ref| per output tensor: TOL of tests/test_gpu_p6.py (f32 1e-3, fp16 1e-3,
bf16 2.5e-2), the bars G2, G4, G5 and G6 are held to."""
import json
import os

import numpy as np
import pytest
import torch

import ghost_case as C
from helpers import rel_err, sd_hash
from test_gpu_p6 import TOL
from ycx import _lib as L
from ycx.nets.yolo import Model
from ycx.utils.synth import synthetic_images, synthetic_state_dict

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope='module')
def g9():
    with open(os.path.join(GOLD, 'g9_ghost.json')) as f:
        meta = json.load(f)
    return meta['gh_mini'], dict(np.load(os.path.join(GOLD, 'g9_ghost.npz')))


def gh_model(precision, meta):
    m = Model(C.gh_mini(), C.ANCHORS2, C.NC, precision=precision).eval()
    sd = synthetic_state_dict(m, seed=C.W_SEED)
    assert sd_hash(sd) == meta['sd_hash']  # the fixture's weights, regenerated
    m.load_state_dict(sd)
    return m


def ghost_ops(eng):
    return [eng.ops[i] for i in range(eng.n_ops) if eng.ops[i].kind == L.OP_GHOST]


@pytest.mark.parametrize('precision', ['f32', 'fp16', 'bf16'])
def test_gh_mini_vs_reference(device, g9, precision):
    meta, gold = g9
    m = gh_model(precision, meta).to(device)
    x = synthetic_images(*C.SHAPE, seed=C.IMG_SEED).to(device)
    z, xs = m(x)
    assert len(xs) == 2 and [C.SHAPE[2] / t.shape[2] for t in xs] == C.STRIDES
    errs = {'z': rel_err(z.cpu(), torch.from_numpy(gold['z']))}
    for j, t in enumerate(xs):
        g = torch.from_numpy(gold[f'x{j}'])
        assert tuple(t.shape) == tuple(g.shape)
        errs[f'x{j}'] = rel_err(t.cpu(), g)
    print(f"\n{precision} G9 gh-mini rel err {errs}")
    assert max(errs.values()) < TOL[precision], errs
    eng = m.engine_for(x.shape, device, slot=m.EAGER_SLOT)
    kinds = [i['kind'] for i in eng.op_info]
    assert kinds.count('ghost') == C.N_GHOST and kinds.count('gconv') == C.N_GCONV
    # the only copy kernel is the upsample under layer 10's GhostConv; no concat slice and no first half is copied
    assert [i['name'] for i in eng.op_info if i['kind'] == 'copy'] == ['upsample2x']
    ops = ghost_ops(eng)
    assert len(ops) == C.N_GHOST
    n_res = 0
    for op in ops:  # plain SiLU or none, fp32 weights, in every precision
        d = op.d.conv
        assert d.cout == 2 * d.cin and d.groups == d.cin and d.kh == 5
        inplace = op.in_ == op.out and d.in_c_off == d.out_c_off and d.in_c_stride == d.out_c_stride
        if op.residual:
            n_res += 1
            assert d.act == L.ACT_NONE and not inplace and op.in_ != op.out
        else:
            assert d.act == L.ACT_SILU and inplace
    assert n_res == C.N_GHOST_RES


@pytest.mark.parametrize('precision', ['bf16', 'fp16'])
def test_gh_graph_replay_matches_eager(device, g9, precision):
    meta, _ = g9
    m = gh_model(precision, meta).to(device)
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


def test_gh_prepack_roundtrip(device, g9, tmp_path):
    """Ghost weights go through the prepack file as fp32 [5][5][c][1], the grouped kernel's packing: saved,
    loaded into a freshly initialised module, the forward is bit-identical."""
    meta, _ = g9
    m = gh_model('bf16', meta).to(device)
    x = synthetic_images(*C.SHAPE, seed=C.IMG_SEED).to(device)
    ref = [o.clone() for o in m.engine_for(x.shape, device).run(x)]
    path = str(tmp_path / 'gh.safetensors')
    m.save_prepacked(path, C.SHAPE[2:], device=device)
    eng = m.engine_for(x.shape, device)
    kinds = ('conv', 'stem', 'stem_reorg', 'gconv', 'deconv', 'ghost')
    gi = next(i for i, nd in enumerate(nd for nd in eng.graph.nodes if nd.kind in kinds) if nd.kind == 'ghost')
    assert eng.packed[f'p{2 * gi}'].dtype == torch.float32 and tuple(eng.packed[f'p{2 * gi}'].shape) == (5, 5, 32, 1)
    m2 = Model(C.gh_mini(), C.ANCHORS2, C.NC, precision='bf16').eval().to(device)  # random weights
    m2.load_prepacked(path)
    for a, b in zip(ref, m2.engine_for(x.shape, device).run(x)):
        assert torch.equal(a, b)


@pytest.mark.parametrize('precision', ['bf16', 'f32'])
def test_gh_chunked_ops_bit_identical(device, g9, precision, monkeypatch):
    """YCX_CHUNK over the whole plan (one image at a time): the ghost ops are image-major like the rest,
    in place or not, so the chunked run equals the unchunked one bit for bit."""
    meta, _ = g9
    m = gh_model(precision, meta).to(device)
    x = synthetic_images(*C.SHAPE, seed=C.IMG_SEED).to(device)
    eng = m.engine_for(x.shape, device)
    eng.bind_static(x)
    whole = [o.clone() for o in eng.run_static()]
    monkeypatch.setenv('YCX_CHUNK', f'1:{eng.n_ops}')
    ops, n_ops = eng._exec_ops()
    assert n_ops == 2 * eng.n_ops and sum(1 for i in range(n_ops) if ops[i].kind == L.OP_GHOST) == 2 * C.N_GHOST
    for a, b in zip(whole, eng.run_static()):
        assert torch.equal(a, b)


def test_gh_fp8_is_refused(device, g9):
    meta, _ = g9
    m = gh_model('fp8', meta).to(device)
    x = synthetic_images(*C.SHAPE, seed=C.IMG_SEED).to(device)
    with pytest.raises(NotImplementedError, match='ghost conv has no fp8 path'):
        m(x)
