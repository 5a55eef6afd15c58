"""The space/depth layers end to end: the sd-mini config (tests/depth_case.py: a Focus stem on the image,
Contract feeding a Conv, Expand into a concat slice, a Focus reading an activation, two-level IDetect) and
its plain-Conv-stem variant through Model.forward against the reference's own eval outputs
(tests/golden/g11_depth.npz, made by tests/golden/make_golden_depth.py).

Bars, max |gpu - ref| / max |ref| per output tensor: TOL of tests/test_gpu_p6.py (f32 1e-3, fp16 1e-3,
bf16 2.5e-2, fp8 0.12), the bars G2, G4, G5, G6 and G9 are held to."""
import json
import os

import numpy as np
import pytest
import torch

import depth_case as C
from helpers import rel_err, sd_hash
from test_gpu_p6 import TOL
from ycx import _lib as L
from ycx.nets.yolo import Model
from ycx.utils.synth import synthetic_images, synthetic_state_dict

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
STEMS = {'focus': ('sd_mini', ''), 'conv': ('sd_mini_conv', 'conv_')}


@pytest.fixture(scope='module')
def g11():
    with open(os.path.join(GOLD, 'g11_depth.json')) as f:
        meta = json.load(f)
    return meta, dict(np.load(os.path.join(GOLD, 'g11_depth.npz')))


def sd_model(precision, meta, stem='focus'):
    m = Model(C.sd_mini(stem), C.ANCHORS2, C.NC, precision=precision).eval()
    sd = synthetic_state_dict(m, seed=C.W_SEED)
    assert sd_hash(sd) == meta[STEMS[stem][0]]['sd_hash']  # the fixture's weights, regenerated
    m.load_state_dict(sd)
    return m


def depth_ops(eng):
    return [eng.ops[i] for i in range(eng.n_ops) if eng.ops[i].kind == L.OP_DEPTH]


def check_outputs(z, xs, gold, prefix, tol, what):
    assert len(xs) == 2 and [C.SHAPE[2] / t.shape[2] for t in xs] == C.STRIDES
    errs = {'z': rel_err(z.cpu(), torch.from_numpy(gold[prefix + 'z']))}
    for j, t in enumerate(xs):
        g = torch.from_numpy(gold[f'{prefix}x{j}'])
        assert tuple(t.shape) == tuple(g.shape)
        errs[f'x{j}'] = rel_err(t.cpu(), g)
    print(f"\n{what} rel err {errs}")
    assert max(errs.values()) < tol, errs


def check_ops(eng, stem):
    """Three depth launches, named by mode and gain, moving as many bytes as they read; no copy kernel: the
    Expand output is stored straight into its slice of the concat buffer."""
    kinds = [i['kind'] for i in eng.op_info]
    assert kinds.count('depth') == C.N_DEPTH and 'copy' not in kinds
    assert kinds.count('stem_reorg') == (1 if stem == 'focus' else 0)
    info = [i for i in eng.op_info if i['kind'] == 'depth']
    assert [i['name'] for i in info] == C.DEPTH_NAMES and all(i['flops'] == 0 for i in info)
    ops = depth_ops(eng)
    assert len(ops) == C.N_DEPTH
    esz = eng.dtype.itemsize
    for op, i in zip(ops, info):
        d = op.d.depth
        assert i['bytes'] == 2 * d.n * d.h * d.w * d.c * esz and d.dtype == eng.dt and op.in_ != op.out
    contract, expand, focus = (op.d.depth for op in ops)
    assert (contract.mode, contract.gain, contract.c, contract.ho) == (L.SD_CONTRACT, 2, 64, 8)
    assert contract.out_c_stride == 256
    assert (expand.mode, expand.gain, expand.c, expand.ho) == (L.SD_EXPAND, 2, 128, 16)
    assert (expand.out_c_off, expand.out_c_stride) == (0, 64)  # the first 32 channels of layer 6's 64-wide concat
    assert (focus.mode, focus.gain, focus.c, focus.in_c_stride, focus.out_c_stride) == (L.SD_FOCUS, 2, 64, 64, 256)
    assert ops[2].in_ == ops[1].out  # the Focus reads the concat buffer the Expand wrote into


@pytest.mark.parametrize('precision', ['f32', 'fp16', 'bf16'])
@pytest.mark.parametrize('stem', ['focus', 'conv'])
def test_sd_mini_vs_reference(device, g11, stem, precision):
    meta, gold = g11
    m = sd_model(precision, meta, stem).to(device)
    x = synthetic_images(*C.SHAPE, seed=C.IMG_SEED).to(device)
    z, xs = m(x)
    check_outputs(z, xs, gold, STEMS[stem][1], TOL[precision], f"{precision} G11 sd-mini ({stem} stem)")
    check_ops(m.engine_for(x.shape, device, slot=m.EAGER_SLOT), stem)


def test_sd_mini_fp8(device, g11):
    """The fp8 plan: a move shares one scale, so every depth op's input and output buffers carry the same one."""
    meta, gold = g11
    m = sd_model('fp8', meta).to(device)
    x = synthetic_images(*C.SHAPE, seed=C.IMG_SEED).to(device)
    z, xs = m(x)
    check_outputs(z, xs, gold, '', TOL['fp8'], "fp8 G11 sd-mini")
    eng = m.engine_for(x.shape, device, slot=m.EAGER_SLOT)
    check_ops(eng, 'focus')
    assert all(t.dtype == torch.float8_e4m3fn for t in eng.buffers)
    nodes = [nd for nd in eng.graph.nodes if nd.kind == 'depth']
    assert len(nodes) == C.N_DEPTH
    for nd in nodes:
        si, so = eng.scales[id(nd.inputs[0].buf)], eng.scales[id(nd.out.buf)]
        assert si == so and si > 0 and np.log2(si) == int(np.log2(si))


@pytest.mark.parametrize('precision', ['bf16', 'fp16'])
def test_sd_graph_replay_matches_eager(device, g11, precision):
    meta, _ = g11
    m = sd_model(precision, meta).to(device)
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


def test_sd_prepack_roundtrip(device, g11, tmp_path):
    """The depth nodes hold no weights: the prepack file numbers the convs as before, and loaded into a
    freshly initialised module the forward is bit-identical."""
    meta, _ = g11
    m = sd_model('bf16', meta).to(device)
    x = synthetic_images(*C.SHAPE, seed=C.IMG_SEED).to(device)
    ref = [o.clone() for o in m.engine_for(x.shape, device).run(x)]
    path = str(tmp_path / 'sd.safetensors')
    m.save_prepacked(path, C.SHAPE[2:], device=device)
    eng = m.engine_for(x.shape, device)
    n_conv = sum(1 for nd in eng.graph.nodes if nd.kind in ('conv', 'stem_reorg'))
    assert len(eng.packed) == 2 * n_conv and tuple(eng.packed['p0'].shape) == (3, 3, 12, 32)  # the Focus stem's conv
    m2 = Model(C.sd_mini(), C.ANCHORS2, C.NC, precision='bf16').eval().to(device)  # random weights
    m2.load_prepacked(path)
    for a, b in zip(ref, m2.engine_for(x.shape, device).run(x)):
        assert torch.equal(a, b)


@pytest.mark.parametrize('name', ['Contract3', 'Expand4', 'Focus_g8'])
def test_single_blocks_run(device, name):
    """A one-block config whose depth output is a model output (through the tonchw copy), and a Focus with a
    grouped conv behind the move: against torch's own view / permute on the block's input."""
    module, args, c_in, op_name = C.SINGLES[name]
    m = Model(C.single(module, args, c_in), C.ANCHORS2, C.NC, precision='f32').eval().to(device)
    x = synthetic_images(*C.SINGLE_SHAPE, seed=C.IMG_SEED).to(device)
    y = m(x)
    eng = m.engine_for(x.shape, device, slot=m.EAGER_SLOT)
    assert [i['name'] for i in eng.op_info if i['kind'] == 'depth'] == [op_name]
    nd = next(nd for nd in eng.graph.nodes if nd.kind == 'depth')
    t = nd.inputs[0].buf.tensor[..., nd.inputs[0].coff:nd.inputs[0].coff + nd.inputs[0].c].permute(0, 3, 1, 2)
    n, c, h, w = t.shape
    s = nd.p['gain']
    if module == 'Contract':   # nets/common.py:793-798
        want = t.reshape(n, c, h // s, s, w // s, s).permute(0, 3, 5, 1, 2, 4).reshape(n, c * s * s, h // s, w // s)
        assert torch.equal(y, want.float())
    elif module == 'Expand':   # nets/common.py:807-812
        want = t.reshape(n, s, s, c // s ** 2, h, w).permute(0, 3, 4, 1, 5, 2).reshape(n, c // s ** 2, h * s, w * s)
        assert torch.equal(y, want.float())
    else:                      # nets/common.py:767, the depth node's own output
        want = torch.cat([t[..., ::2, ::2], t[..., 1::2, ::2], t[..., ::2, 1::2], t[..., 1::2, 1::2]], 1)
        got = nd.out.buf.tensor[..., nd.out.coff:nd.out.coff + nd.out.c].permute(0, 3, 1, 2)
        assert torch.equal(got, want) and tuple(y.shape) == (1, 64, 12, 12)
        assert [i['kind'] for i in eng.op_info].count('gconv') == 1
