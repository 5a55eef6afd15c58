"""P6 networks end to end: the p6-mini config (tests/p6_case.py: ReOrg stem, DownC stages, SPPCSPC,
four-level IDetect / IAuxDetect) through Model.forward against the reference's own eval outputs
(tests/golden/g5_p6.npz, made by tests/golden/make_golden_p6.py).

Bars, max |gpu - ref| / max |ref| per output tensor, as tests/test_gpu_model.py holds G2 / G4 to:
f32 1e-3, fp16 1e-3, bf16 2.5e-2; fp8 as tests/test_gpu_fp8.py: 0.12."""
import json
import os

import numpy as np
import pytest
import torch

import p6_case as P
from helpers import rel_err, sd_hash
from ycx.nets.yolo import Model
from ycx.utils.synth import synthetic_images, synthetic_state_dict

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
TOL = {'f32': 1e-3, 'fp16': 1e-3, 'bf16': 2.5e-2, 'fp8': 0.12}
ROWS = [3 * s * s for s in (16, 8, 4, 2)]


@pytest.fixture(scope='module')
def g5():
    with open(os.path.join(GOLD, 'g5_p6.json')) as f:
        meta = json.load(f)
    return meta, dict(np.load(os.path.join(GOLD, 'g5_p6.npz')))


def p6_model(name, precision, meta):
    m = Model(P.p6_mini(P.VARIANTS[name]), P.ANCHORS4, P.NC, precision=precision).eval()
    sd = synthetic_state_dict(m, seed=P.W_SEED)
    assert sd_hash(sd) == meta[name]['sd_hash']  # the fixture's weights, regenerated
    m.load_state_dict(sd)
    return m


def check_outputs(z, xs, gold, name, tol, what):
    assert len(xs) == 4 and tuple(z.shape) == (2, sum(ROWS), P.NC + 5) and sum(ROWS) == 3 * (16 ** 2 + 8 ** 2 + 4 ** 2 + 2 ** 2)
    assert [P.SHAPE[2] / x.shape[2] for x in xs] == P.STRIDES
    zr = torch.from_numpy(gold[f'{name}/z'])
    errs = {'z': rel_err(z.cpu(), zr)}
    for j, x in enumerate(xs):
        g = torch.from_numpy(gold[f'{name}/x{j}'])
        assert tuple(x.shape) == tuple(g.shape)
        errs[f'x{j}'] = rel_err(x.cpu(), g)
    # the stride-64 level's boxes on their own (the last 12 rows; pixels, anchors up to 925)
    lvl4 = slice(sum(ROWS[:3]), sum(ROWS))
    errs['z_stride64_box'] = rel_err(z.cpu()[:, lvl4, :4], zr[:, lvl4, :4])
    errs['z_stride64_conf'] = rel_err(z.cpu()[:, lvl4, 4:], zr[:, lvl4, 4:])
    print(f"\n{what} rel err {errs}")
    assert max(errs.values()) < tol, errs


@pytest.mark.parametrize('precision', ['f32', 'fp16', 'bf16'])
@pytest.mark.parametrize('name', list(P.VARIANTS))
def test_p6_mini_vs_reference(device, g5, name, precision):
    meta, gold = g5
    m = p6_model(name, precision, meta).to(device)
    x = synthetic_images(*P.SHAPE, seed=P.IMG_SEED).to(device)
    z, xs = m(x)
    check_outputs(z, xs, gold, name, TOL[precision], f"{precision} G5 {name}")
    eng = m.engine_for(x.shape, device, slot=m.EAGER_SLOT)
    kinds = [i['kind'] for i in eng.op_info]
    assert kinds.count('stem_reorg') == 1 and 'stem' not in kinds and 'stem2' not in kinds and 'copy' not in kinds
    # the four main heads and nothing of the aux branch: 4 head convs read from 4 maps
    assert len(eng.out_vals) == 4 and [(v.h, v.w) for v in eng.out_vals] == [(16, 16), (8, 8), (4, 4), (2, 2)]
    if name == 'iauxdetect':
        assert eng.n_ops == p6_model('idetect', precision, meta).to(device).engine_for(x.shape, device).n_ops
    if precision != 'f32':  # every DownC pool runs inside its 1x1 conv
        assert sum(1 for i in eng.op_info if i['name'].endswith('+maxpool_k2s2')) == 4


def test_p6_mini_fp8(device, g5):
    meta, gold = g5
    m = p6_model('idetect', 'fp8', meta).to(device)
    x = synthetic_images(*P.SHAPE, seed=P.IMG_SEED).to(device)
    z, xs = m(x)
    check_outputs(z, xs, gold, 'idetect', TOL['fp8'], "fp8 G5 idetect")
    eng = m.engine_for(x.shape, device, slot=m.EAGER_SLOT)
    assert [i['kind'] for i in eng.op_info].count('stem_reorg') == 1
    assert all(t.dtype == torch.float8_e4m3fn for t in eng.buffers)


@pytest.mark.parametrize('precision', ['bf16', 'fp16'])
def test_p6_graph_replay_matches_eager(device, g5, precision):
    meta, _ = g5
    m = p6_model('idetect', precision, meta).to(device)
    x = synthetic_images(*P.SHAPE, seed=P.IMG_SEED).to(device)
    eng = m.engine_for(x.shape, device)
    eager = [o.clone() for o in eng.run(x)]
    _, outs = eng.bind_static(x)
    eng.capture()
    first = [o.clone() for o in eng.replay()]
    torch.cuda.synchronize()
    second = eng.replay()
    torch.cuda.synchronize()
    for a, b, c in zip(eager, first, second):
        assert torch.equal(a, b) and torch.equal(b, c)


def test_p6_prepack_roundtrip(device, g5, tmp_path):
    """A plan with a stem_reorg packs its fp32 stem weights as the stem node does: saved, loaded
    into a fresh module with other parameters, the forward is bit-identical."""
    meta, _ = g5
    m = p6_model('idetect', 'bf16', meta).to(device)
    x = synthetic_images(*P.SHAPE, seed=P.IMG_SEED).to(device)
    ref = [o.clone() for o in m.engine_for(x.shape, device).run(x)]
    path = str(tmp_path / 'p6.safetensors')
    m.save_prepacked(path, P.SHAPE[2:], device=device)
    eng = m.engine_for(x.shape, device)
    assert eng.packed['p0'].dtype == torch.float32 and tuple(eng.packed['p0'].shape) == (3, 3, 12, 64)
    m2 = Model(P.p6_mini('IDetect'), P.ANCHORS4, P.NC, precision='bf16').eval().to(device)  # random weights
    m2.load_prepacked(path)
    for a, b in zip(ref, m2.engine_for(x.shape, device).run(x)):
        assert torch.equal(a, b)


@pytest.mark.parametrize('precision', ['f32', 'fp16', 'bf16'])
def test_downc_block(device, g5, precision):
    """DownC alone (k2 pool) against the reference's block output; in the 16-bit plans the pooled
    1x1 (cv3 on the max-pool) runs fused and, with fuse_pool=False, apart: bit-identical results."""
    from ycx.engine import Engine
    meta, gold = g5
    m = Model(P.downc_block(), P.ANCHORS4, P.NC, precision=precision).eval()
    sd = synthetic_state_dict(m, seed=P.DOWNC_W_SEED)
    assert sd_hash(sd) == meta['downc']['sd_hash']
    m.load_state_dict(sd)
    m.to(device)
    x = synthetic_images(*P.DOWNC_SHAPE, seed=P.DOWNC_IMG_SEED).to(device)
    ref = torch.from_numpy(gold['downc/0'])
    outs = []
    for fuse in (True, False):
        eng = Engine(m, tuple(x.shape), torch.device(device), precision, fuse_pool=fuse)
        try:
            fused = sum(1 for i in eng.op_info if i['name'].endswith('+maxpool_k2s2'))
            assert fused == (1 if fuse and precision != 'f32' else 0)
            assert sum(1 for i in eng.op_info if i['kind'] == 'pool') == 1 - fused
            outs.append(eng.run(x).clone())
        finally:
            eng.close()
    err = rel_err(outs[0].cpu(), ref)
    print(f"\n{precision} DownC block rel err {err:.5f}")
    assert tuple(outs[0].shape) == tuple(ref.shape) and err < TOL[precision]
    assert torch.equal(outs[0], outs[1])
