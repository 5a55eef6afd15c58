"""Host-side (CPU) checks of the IBin head: the builder against the reference's bookkeeping and the head
module's state_dict schema (tests/golden/g12_ibin.json), the two head convs of the plan with ImplicitA / M
folded (against the unfolded formula in float64), their packed widths and tiles in every precision, the
bin_count refusal, and ycx_ibin_decode's argument validation (no device call is made)."""
import ctypes
import hashlib
import json
import os
import warnings

import pytest
import torch

import ibin_case as C
from ycx import _lib as L
from ycx.engine import Plan, check_plan_precision
from ycx.nets.detect import IBin, IDetect, SigmoidBin
from ycx.nets.yolo import Model, parse_model
from ycx.schedule import Schedule, cout_pad
from ycx.utils.synth import synthetic_state_dict

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope='module')
def g12():
    with open(os.path.join(GOLD, 'g12_ibin.json')) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def model():
    m = Model(C.ibin_mini(), C.ANCHORS2, C.NC).eval()
    m.load_state_dict(synthetic_state_dict(m, seed=C.W_SEED))
    return m


def test_parse_model_builds_ibin_like_the_reference(g12):
    """Fails on a tree without the feature: 'IBin' raises "out of scope" at parse time there."""
    layers, save = parse_model(C.ibin_mini(), [3], C.ANCHORS2, C.NC)
    assert len(layers) == g12['n_layers'] and save == g12['save']
    assert sum(p.numel() for p in layers.parameters()) == g12['n_params']
    head = layers[-1]
    assert type(head) is IBin and not isinstance(head, IDetect) and head.stride is None
    assert (head.no, head.nl, head.na, head.nc, head.bin_count) == (C.NO, 2, C.NA, C.NC, C.BIN_COUNT) == \
        (g12['no'], 2, 3, g12['nc'], g12['bin_count'])
    assert [m.in_channels for m in head.m] == [128, 128] and all(m.out_channels == C.NA * C.NO for m in head.m)
    m = Model(C.ibin_mini(), C.ANCHORS2, C.NC)
    sd = m.state_dict()
    assert len(sd) == g12['n_keys']
    assert hashlib.sha256('\n'.join(sorted(sd.keys())).encode()).hexdigest() == g12['keys_sha256']


def test_head_state_dict_schema(g12):
    """The reference module's own keys, order and shapes, the two SigmoidBin children's included."""
    head = IBin(C.NC, C.ANCHORS2, (128, 128))
    sd = head.state_dict()
    assert list(sd) == list(g12['head_state_dict'])
    assert {k: list(v.shape) for k, v in sd.items()} == g12['head_state_dict']
    for k in ('w_bin_sigmoid.bins', 'h_bin_sigmoid.bins'):
        assert list(sd[k].shape) == [C.BIN_COUNT] and sd[k].dtype == torch.float32
    for k in ('w_bin_sigmoid.BCE_bins.pos_weight', 'h_bin_sigmoid.BCE_bins.pos_weight'):
        assert sd[k].tolist() == [1.0]
    # the bin centres: torch.range(start, end + 0.0001, step).float() over [0, 4], 21 of them
    step = 4.0 / 21
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        want = torch.range(step / 2, 4.0 - step / 2 + 0.0001, step).float()
    assert torch.equal(head.w_bin_sigmoid.bins, want) and torch.equal(head.h_bin_sigmoid.bins, want)
    assert head.w_bin_sigmoid.step == step and head.w_bin_sigmoid.get_length() == C.BIN_COUNT + 1
    assert SigmoidBin(10).bins.numel() == 10  # the reference's default


def test_integer_anchor_count_is_expanded():
    layers, _ = parse_model(C.ibin_mini(), [3], 3, C.NC)
    assert layers[-1].na == 3 and layers[-1].nl == 2 and tuple(layers[-1].anchors.shape) == (2, 3, 2)


def test_synthetic_state_dict_loads_strictly(g12, model):
    from helpers import sd_hash
    m = Model(C.ibin_mini(), C.ANCHORS2, C.NC)
    sd = synthetic_state_dict(m, seed=C.W_SEED)
    assert sd_hash(sd) == g12['sd_hash']  # the fixture's weights, regenerated
    r = m.load_state_dict(sd, strict=True)
    assert not r.missing_keys and not r.unexpected_keys


def test_bin_count_other_than_21_is_refused():
    for bc in (10, 20, 22):
        with pytest.raises(NotImplementedError, match=r'bin_count == 21 only'):
            IBin(C.NC, C.ANCHORS2, (128, 128), bin_count=bc)
    assert IBin(C.NC, C.ANCHORS2, (128, 128), bin_count=21).no == C.NO


def test_plan_has_two_folded_head_convs(model):
    plan = Plan(model, C.SHAPE)
    assert plan.counts() == {'stem': 1, 'conv': 5}
    assert [(v.n, v.h, v.w, v.c) for v in plan.out_vals] == [(2, 8, 8, C.NA * C.NO), (2, 4, 4, C.NA * C.NO)]
    head = model.model[-1]
    heads = [v.producer for v in plan.out_vals]
    for i, nd in enumerate(heads):
        assert nd.kind == 'conv' and nd.p['layout'] == L.OUT_NCHW_F32 and nd.p['act'] == L.ACT_NONE
        assert (nd.p['k'], nd.p['s'], nd.p['p']) == (1, 1, 0) and nd.out.role == 'output'
        w, b = nd.p['w'], nd.p['b']
        assert w.dtype == torch.float64 and tuple(w.shape) == (C.NA * C.NO, 128, 1, 1)
        # im * conv(x + ia) on a float64 probe, unfolded (nets/ibin.py:46-47), against the folded conv
        g = torch.Generator().manual_seed(5 + i)
        x = torch.randn(2, 128, 3, 4, generator=g, dtype=torch.float64)
        cw, cb = head.m[i].weight.detach().double(), head.m[i].bias.detach().double()
        want = torch.nn.functional.conv2d(x + head.ia[i].implicit.detach().double(), cw, cb) * \
            head.im[i].implicit.detach().double()
        got = torch.nn.functional.conv2d(x, w, b)
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
        assert not torch.equal(w, cw) and not torch.equal(b, cb)  # the fold is not the identity here


@pytest.mark.parametrize('nc, width', [(C.NC, 150), (C.NC_WIDE, 381)])
def test_head_width_packs_and_schedules_in_every_precision(nc, width):
    """Widths no earlier head had: 150 and 381 channels. cout_pad rounds them to whole tiles (128-row tiles
    in the 16-bit plans, 64-row in f32 and fp8), and no precision is refused."""
    m = Model(C.ibin_mini(), C.ANCHORS2, nc).eval()
    assert m.model[-1].no * C.NA == width
    plan = Plan(m, C.SHAPE)
    assert [v.c for v in plan.out_vals] == [width, width]
    want = {'bf16': -(-width // 128) * 128, 'fp16': -(-width // 128) * 128, 'f32': -(-width // 64) * 64,
            'fp8': -(-width // 64) * 64}
    for prec, pad in want.items():
        check_plan_precision(plan, prec)
        assert cout_pad(prec, width) == pad and pad >= width
        kinds = [la.kind for la in Schedule(plan, prec).launches]
        assert 'copy' not in kinds and 'tonchw' not in kinds
    # the tile the library picks for such a head conv is one of its cout_pad-generic ones
    for prec, dt in (('bf16', L.DT_BF16), ('f32', L.DT_F32), ('fp8', L.DT_FP8)):
        for hw in (8, 4):
            d = L.ConvDesc()
            d.n, d.h, d.w, d.ho, d.wo, d.cin, d.in_c_stride, d.cout, d.cout_pad = 2, hw, hw, hw, hw, 128, 128, width, want[prec]
            d.kh = d.kw = d.stride = 1
            d.dtype, d.out_layout = dt, L.OUT_NCHW_F32
            tile = int(L.lib.ycx_conv_pick_tile(ctypes.byref(d)))
            assert tile > 0 and L.lib.ycx_conv_tile_name(tile) != b'invalid'


def ddesc(no=C.NO, na=C.NA, h=5, w=7, n=2, row_off=0, extra_rows=0):
    d = L.DecodeDesc()
    d.n, d.h, d.w, d.na, d.no, d.row_off = n, h, w, na, no, row_off
    d.rows_total = row_off + na * h * w + extra_rows
    for a in range(min(2 * na, 16)):
        d.anchors_scaled[a] = 10.0 + a
    return d


def bad_descs():
    """Descriptors ycx_ibin_decode answers with YCX_ERR_BAD_ARG at bin_count 21."""
    bad = []
    for f in ('n', 'h', 'w', 'na', 'no'):
        for v in (0, -1):
            d = ddesc(); setattr(d, f, v); bad.append(d)
    d = ddesc(no=2 * (C.BIN_COUNT + 1) + 3); bad.append(d)        # no class column
    d = ddesc(no=5); bad.append(d)                                  # an IDetect width
    d = ddesc(); d.row_off = -1; bad.append(d)
    d = ddesc(); d.rows_total -= 1; bad.append(d)                   # the level does not fit
    d = ddesc(row_off=8); d.rows_total -= 8; bad.append(d)
    d = ddesc(); d.rows_total = 0; bad.append(d)
    return bad


def test_ibin_decode_entry_point_validates_before_any_device_call():
    """Every call here must return before a launch: the data pointers are null or host memory."""
    assert L.ABI_VERSION == 9 and L.lib.ycx_abi_version() == 9 and 'ycx_ibin_decode' in L.SYMBOLS
    assert len(L._STRUCTS) == 12 and L.lib.ycx_struct_size(12) == 0  # no new struct
    bins = (ctypes.c_float * C.BIN_COUNT)(*[0.1 * k for k in range(C.BIN_COUNT)])
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)

    def call(d, bc=C.BIN_COUNT, wb=bins, hb=bins, head=None, z=None, xv=None):
        return L.lib.ycx_ibin_decode(ctypes.byref(d) if d is not None else None, ctypes.c_float(8.0), bc, wb, hb,
                                     head, z, xv, None)

    assert call(None) == L.YCX_ERR_BAD_ARG
    assert call(L.DecodeDesc()) == L.YCX_ERR_BAD_ARG  # the empty descriptor
    # a good descriptor: each null pointer alone is a bad argument (the others are host memory, never read)
    for null in ('wb', 'hb', 'head', 'z', 'xv'):
        kw = dict(wb=bins, hb=bins, head=p, z=p, xv=p)
        kw[null] = None
        assert call(ddesc(), **kw) == L.YCX_ERR_BAD_ARG
        assert call(ddesc(no=127, row_off=64, extra_rows=9), **kw) == L.YCX_ERR_BAD_ARG
    for d in bad_descs():
        assert call(d) == L.YCX_ERR_BAD_ARG
        assert call(d, head=p, z=p, xv=p) == L.YCX_ERR_BAD_ARG
    for bc in (0, -21):
        assert call(ddesc(), bc=bc) == L.YCX_ERR_BAD_ARG
    # unsupported: the descriptor is judged before the data pointers (all null here)
    for bc in (1, 10, 20, 22, 64):
        assert call(ddesc(no=C.NC + 3 + 2 * (bc + 1)), bc=bc) == L.YCX_ERR_UNSUPPORTED
    assert call(ddesc(na=9)) == L.YCX_ERR_UNSUPPORTED
    assert call(ddesc(no=257)) == L.YCX_ERR_UNSUPPORTED
    assert call(ddesc(n=65536)) == L.YCX_ERR_UNSUPPORTED
    assert call(ddesc(no=256)) == L.YCX_ERR_BAD_ARG  # a width it takes: now the null pointers are what is wrong


def test_torch_restatement_equals_the_reference(g12):
    """The restatement the GPU tests compare against (tests/test_gpu_ibin_decode.py), applied to the
    reference's own raw maps, gives the reference's own z bit for bit (CPU torch on both sides)."""
    import numpy as np
    from test_gpu_ibin_decode import ibin_rows_ref, near_tie
    gold = np.load(os.path.join(GOLD, 'g12_ibin.npz'))
    head = IBin(C.NC, C.ANCHORS2, (128, 128))
    zs, tied = [], 0
    for i in range(g12['n_x']):
        x = torch.from_numpy(gold[f'x{i}'])
        z, p = ibin_rows_ref(x, C.ANCHORS2[i], g12['strides'][i], head.w_bin_sigmoid.bins, head.h_bin_sigmoid.bins)
        zs.append(z)
        tied += int(near_tie(p).any(1).sum())
    z = torch.cat(zs, 1)
    assert tuple(z.shape) == (C.SHAPE[0], sum(C.ROWS), C.NZ)
    assert torch.equal(z, torch.from_numpy(gold['z']))
    assert tied <= 0.01 * g12['rows']


def test_existing_heads_keep_their_branch():
    """IDetect and IAuxDetect still take idetect_outputs: IBin is no subclass of either, nor they of it."""
    from ycx.nets.detect import IAuxDetect
    assert not issubclass(IBin, IDetect) and not issubclass(IDetect, IBin) and not issubclass(IAuxDetect, IBin)
    with pytest.raises(NotImplementedError, match='out of scope'):
        parse_model({'depth_multiple': 1.0, 'width_multiple': 1.0, 'head': [],
                     'backbone': [[-1, 1, 'TransformerBlock', [64]]]}, [3], C.ANCHORS2, C.NC)
