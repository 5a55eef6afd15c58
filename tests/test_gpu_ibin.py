"""The IBin head end to end: the ibin-mini config (tests/ibin_case.py: four Convs to strides 8 and 16, a
two-level IBin head, nc 3 so no = 50) through Model.forward against the reference's own eval outputs
(tests/golden/g12_ibin.npz, made by tests/golden/make_golden_ibin.py).

Raw maps xs: max |gpu - ref| / max |ref| per tensor under TOL of tests/test_gpu_p6.py (f32 1e-3, fp16 1e-3,
bf16 2.5e-2, fp8 0.12).

Decoded rows z: against the torch restatement of tests/test_gpu_ibin_decode.py applied to the engine's OWN
xs, under that file's tolerance and near-tie skip rule, so a bin flipped by the convs' rounding is not
charged to the decode. In f32 also against the golden z under the f32 bar, leaving out w / h of the rows
whose golden top-two bin logits are closer than that bar times the row's largest |logit| (at most 1 % of
the rows; the generator asserts the same of the golden itself)."""
import json
import os

import numpy as np
import pytest
import torch

import ibin_case as C
from helpers import rel_err, sd_hash
from test_gpu_ibin_decode import MAX_SKIPPED, compare_z, ibin_rows_ref
from test_gpu_p6 import TOL
from ycx.nets.yolo import Model
from ycx.utils.synth import synthetic_images, synthetic_state_dict

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope='module')
def g12():
    with open(os.path.join(GOLD, 'g12_ibin.json')) as f:
        meta = json.load(f)
    return meta, dict(np.load(os.path.join(GOLD, 'g12_ibin.npz')))


def ibin_model(precision, meta=None, nc=C.NC):
    m = Model(C.ibin_mini(), C.ANCHORS2, nc, precision=precision).eval()
    sd = synthetic_state_dict(m, seed=C.W_SEED)
    if meta is not None:
        assert sd_hash(sd) == meta['sd_hash']  # the fixture's weights, regenerated
    m.load_state_dict(sd)
    return m


def restated_z(head, xs):
    """The torch restatement on raw maps (CPU, (n, na, ny, nx, no) each): (cat z, cat of the sigmoid'd scores)."""
    zs, ps = [], []
    for i, x in enumerate(xs):
        z, p = ibin_rows_ref(x, head.anchors[i].reshape(-1).tolist(), C.STRIDES[i],
                             head.w_bin_sigmoid.bins.cpu(), head.h_bin_sigmoid.bins.cpu())
        zs.append(z)
        ps.append(p.reshape(p.shape[0], -1, p.shape[-1]))
    return torch.cat(zs, 1), torch.cat(ps, 1)


def check_shapes(z, xs, nc=C.NC):
    no = nc + 3 + 2 * (C.BIN_COUNT + 1)
    assert tuple(z.shape) == (C.SHAPE[0], sum(C.ROWS), nc + 5) and z.dtype == torch.float32
    assert len(xs) == 2 and [C.SHAPE[2] / t.shape[2] for t in xs] == C.STRIDES
    assert [tuple(t.shape) for t in xs] == [(C.SHAPE[0], C.NA, 8, 8, no), (C.SHAPE[0], C.NA, 4, 4, no)]


@pytest.mark.parametrize('precision', ['f32', 'fp16', 'bf16', 'fp8'])
def test_ibin_mini_vs_reference(device, g12, precision):
    meta, gold = g12
    m = ibin_model(precision, meta).to(device)
    x = synthetic_images(*C.SHAPE, seed=C.IMG_SEED).to(device)
    z, xs = m(x)
    check_shapes(z, xs)
    # raw logits against the reference's
    errs = {}
    for j, t in enumerate(xs):
        g = torch.from_numpy(gold[f'x{j}'])
        assert tuple(t.shape) == tuple(g.shape)
        errs[f'x{j}'] = rel_err(t.cpu(), g)
    print(f"\n{precision} G12 ibin-mini raw maps rel err {errs}")
    assert max(errs.values()) < TOL[precision], errs
    # decoded rows against the restatement on the engine's own logits
    head = m.model[-1]
    z_own, p_own = restated_z(head, [t.cpu() for t in xs])
    compare_z(z.cpu(), z_own, p_own, f"{precision} G12 ibin-mini z vs the restatement on its own logits")
    eng = m.engine_for(x.shape, device, slot=m.EAGER_SLOT)
    assert [(v.h, v.w, v.c) for v in eng.out_vals] == [(8, 8, C.NA * C.NO), (4, 4, C.NA * C.NO)]
    if precision == 'fp8':
        assert all(t.dtype == torch.float8_e4m3fn for t in eng.buffers)
    if precision != 'f32':
        return
    # f32: the decoded rows against the reference's own z
    gz = torch.from_numpy(gold['z'])
    gx = torch.cat([torch.from_numpy(gold[f'x{j}']).reshape(C.SHAPE[0], -1, C.NO) for j in range(2)], 1)
    scale = gx.abs().amax(-1) * TOL['f32']
    skip = []
    for lo in (3, 4 + C.BIN_COUNT):
        top = gx[..., lo:lo + C.BIN_COUNT].topk(2, -1).values
        skip.append((top[..., 0] - top[..., 1]) < scale)
    skip = torch.stack(skip, -1)  # (n, rows, 2)
    assert int(skip.any(-1).sum()) == meta['near_tie_rows'] <= MAX_SKIPPED * meta['rows']
    zc, fig = z.cpu(), {}
    for name, cols in (('xy', [0, 1]), ('conf', list(range(4, C.NZ)))):
        fig[name] = rel_err(zc[..., cols], gz[..., cols])
    for j, name in enumerate(('w', 'h')):
        keep = ~skip[..., j]
        fig[name] = rel_err(zc[..., 2 + j][keep], gz[..., 2 + j][keep])
    print(f"\nf32 G12 ibin-mini z vs the reference's z {fig}, skipped rows {int(skip.any(-1).sum())}")
    assert max(fig.values()) < TOL['f32'], fig


@pytest.mark.parametrize('precision', ['f32', 'bf16'])
def test_ibin_wide_head(device, precision):
    """nc = 80: head convs 381 channels wide (cout_pad 384), no = 127 (64 cells fill the decode's LDS). The raw
    maps against a float64 torch forward of the same modules, z against the restatement on the engine's own."""
    m = ibin_model(precision, nc=C.NC_WIDE).to(device)
    x = synthetic_images(*C.SHAPE, seed=C.IMG_SEED).to(device)
    z, xs = m(x)
    check_shapes(z, xs, C.NC_WIDE)
    head = m.model[-1]
    t, feats = x.cpu().double(), []
    for layer in list(m.model)[:-1]:  # Conv = SiLU(bn(conv(x))), BN in eval mode
        cv, bn = layer.conv, layer.bn
        t = torch.nn.functional.conv2d(t, cv.weight.detach().cpu().double(), None, cv.stride, cv.padding)
        t = torch.nn.functional.batch_norm(t, bn.running_mean.cpu().double(), bn.running_var.cpu().double(),
                                           bn.weight.detach().cpu().double(), bn.bias.detach().cpu().double(), False, 0.0, bn.eps)
        t = torch.nn.functional.silu(t)
        feats.append(t)
    errs = {}
    for i, src in enumerate(C.OUT_LAYERS):
        cv = head.m[i]
        r = torch.nn.functional.conv2d(feats[src] + head.ia[i].implicit.detach().cpu().double(),
                                       cv.weight.detach().cpu().double(), cv.bias.detach().cpu().double())
        r = r * head.im[i].implicit.detach().cpu().double()
        n, _, ny, nx = r.shape
        r = r.view(n, C.NA, head.no, ny, nx).permute(0, 1, 3, 4, 2)
        errs[f'x{i}'] = rel_err(xs[i].cpu(), r)
    print(f"\n{precision} ibin-mini nc=80 raw maps rel err {errs}")
    assert max(errs.values()) < TOL[precision], errs
    z_own, p_own = restated_z(head, [t.cpu() for t in xs])
    compare_z(z.cpu(), z_own, p_own, f"{precision} ibin-mini nc=80 z vs the restatement on its own logits")


def test_ibin_default_stride_is_image_over_grid(device, g12):
    """head.stride unset (the reference's state): stride_i = input height / ny_i, here the fixture's 8 and 16."""
    meta, _ = g12
    m = ibin_model('f32', meta).to(device)
    x = synthetic_images(*C.SHAPE, seed=C.IMG_SEED).to(device)
    assert m.model[-1].stride is None
    z0, _ = m(x)
    m.model[-1].stride = torch.tensor(C.STRIDES)
    z1, _ = m(x)
    assert torch.equal(z0, z1)
    m.model[-1].stride = torch.tensor([4.0, 4.0])
    z2, _ = m(x)
    assert not torch.equal(z0[..., :2], z2[..., :2]) and torch.equal(z0[..., 2:], z2[..., 2:])


@pytest.mark.parametrize('precision', ['bf16', 'fp16'])
def test_ibin_graph_replay_matches_eager(device, g12, precision):
    meta, _ = g12
    m = ibin_model(precision, meta).to(device)
    x = synthetic_images(*C.SHAPE, seed=C.IMG_SEED).to(device)
    eng = m.engine_for(x.shape, device)
    eager = [o.clone() for o in eng.run(x)]
    eng.bind_static(x)
    eng.capture()
    first = [o.clone() for o in eng.replay()]
    torch.cuda.synchronize()
    second = eng.replay()
    torch.cuda.synchronize()
    assert len(eager) == 2 and tuple(eager[0].shape) == (C.SHAPE[0], C.NA * C.NO, 8, 8)
    for a, b, c in zip(eager, first, second):
        assert torch.equal(a, b) and torch.equal(b, c)


def test_ibin_prepack_roundtrip(device, g12, tmp_path):
    """The head convs are ordinary head convs: saved and loaded into a freshly initialised module, the head
    maps and the decoded rows are bit-identical."""
    meta, _ = g12
    m = ibin_model('bf16', meta).to(device)
    x = synthetic_images(*C.SHAPE, seed=C.IMG_SEED).to(device)
    z_ref, xs_ref = m(x)
    ref = [o.clone() for o in m.engine_for(x.shape, device).run(x)]
    path = str(tmp_path / 'ibin.safetensors')
    m.save_prepacked(path, C.SHAPE[2:], device=device)
    m2 = Model(C.ibin_mini(), C.ANCHORS2, C.NC, precision='bf16').eval().to(device)  # random weights
    m2.load_prepacked(path)
    for a, b in zip(ref, m2.engine_for(x.shape, device).run(x)):
        assert torch.equal(a, b)
    z2, xs2 = m2(x)
    assert torch.equal(z_ref, z2) and all(torch.equal(a, b) for a, b in zip(xs_ref, xs2))


def test_fp16_range_guard_reaches_the_ibin_branch(device, g12):
    """An activation past the fp16 range: the forward warns, re-plans in bf16 and still returns (z, xs)."""
    meta, _ = g12
    m = ibin_model('fp16', meta)
    with torch.no_grad():
        m.model[0].bn.weight.mul_(1e6)
    m.invalidate(weights_changed=True)
    m.to(device)
    x = synthetic_images(*C.SHAPE, seed=C.IMG_SEED).to(device)
    with pytest.warns(RuntimeWarning, match='fp16 plan overflowed'):
        z, xs = m(x)
    assert m.precision == 'bf16'
    check_shapes(z, xs)
