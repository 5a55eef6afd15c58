"""Host-side helpers against the oracle (CPU only, no GPU calls)."""
import numpy as np
import pytest

from oracle import ref_post
from ycx.detect import yolo_correct_boxes


@pytest.mark.parametrize('letterbox', [True, False])
@pytest.mark.parametrize('image_hw', [(512, 773), (640, 640), (1080, 1920), (333, 17)])
def test_yolo_correct_boxes_matches_oracle(letterbox, image_hw):
    """The host yolo_correct_boxes (detect.py:147-165) reproduces the reference's
    numpy arithmetic bit for bit, including the in-place float32 scaling of the
    caller's box_wh."""
    rng = np.random.default_rng(sum(image_hw) + letterbox)
    xy = rng.random((257, 2), dtype=np.float32)
    wh = rng.random((257, 2), dtype=np.float32) * np.float32(0.5)
    wh_a, wh_b = wh.copy(), wh.copy()
    got = yolo_correct_boxes(xy.copy(), wh_a, (640, 640), np.array(image_hw), letterbox)
    want = ref_post.yolo_correct_boxes(xy.copy(), wh_b, (640, 640), np.array(image_hw), letterbox)
    assert got.dtype == want.dtype and got.shape == want.shape == (257, 4)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(wh_a, wh_b)  # the same in-place side effect on the caller's array


def test_target_box_record():
    """utils/target_box.py:8-38 API: corner fields, accessors, printable record;
    the palette of utils/helper_cv.py:60-64."""
    from ycx.utils.target_box import TargetBox, colors_for
    tb = TargetBox([3, 4, 50, 60], 0.75, 'dog', (255, 0, 0))
    assert (tb.left, tb.top, tb.right, tb.bottom) == (3, 4, 50, 60)
    assert tb.get_topleft() == (3, 4) and tb.get_bottomright() == (50, 60)
    text = str(tb)
    assert text.startswith('-' * 20 + 'TargetBox') and 'dog' in text and '0.75' in text
    assert colors_for(3) == [(255, 0, 0), (0, 255, 0), (0, 0, 255)]
    assert colors_for(1) == [(255, 0, 0)]



def test_decoded_flip_report_attribution():
    """helpers.decoded_flip_report (the fp16 C1 predict attribution): identical decoded
    tensors give no flips; a score swap between two overlapping boxes flips both keep
    decisions and is attributed to the swap; a score moved across conf_thres is a
    membership flip next to the threshold."""
    import torch
    from helpers import decoded_flip_report
    d = torch.tensor([[0.50, 0.50, 0.20, 0.20, 0.90, 0.90],    # row 0: kept
                      [0.51, 0.50, 0.20, 0.20, 0.89, 0.90],    # row 1: suppressed by 0
                      [0.10, 0.10, 0.05, 0.05, 0.60, 0.50],    # row 2: score 0.30, at conf
                      [0.90, 0.90, 0.05, 0.05, 0.80, 0.80]])   # row 3: alone
    r = decoded_flip_report(d, d, 1, 0.3, 0.3)
    assert r['keep_flips'] == 0 and r['member_flips'] == 0 and r['unexplained_flips'] == 0
    e = d.clone()
    e[1, 4] = 0.91  # row 1 now outranks row 0: the kept box changes (two flips, one class)
    e[2, 4] = 0.599  # score 0.2995: below conf on the device side only
    r = decoded_flip_report(e, d, 1, 0.3, 0.3)
    assert r['keep_flips'] == 3 and r['member_flips'] == 1 and r['member_far'] == 0, r
    assert r['unexplained_flips'] == 0 and r['flip_classes'] == 1, r


@pytest.mark.parametrize('dtype_name', ['bfloat16', 'float16'])
def test_exact_comparator_bites(dtype_name):
    """The comparator of tests/test_gpu_conv_exact.py (bit patterns against helpers.rne of the float64
    sum, distances by helpers.elt_ulps) on a cin 64, 3x3 reference: it must report each of
    (a) truncation toward zero in place of RNE, (b) round-half-away in place of ties-to-even, (c) one
    dropped term of magnitude 1/16, (d) slope 0.1 where the descriptor says 0.125 -- and nothing on
    the correctly rounded result."""
    import torch
    import torch.nn.functional as F
    from helpers import dyadic, elt_neighbours, elt_ulps, rne, rounding_stats
    tdt = getattr(torch, dtype_name)
    sx, sw = (1 / 4, 1 / 4) if tdt == torch.bfloat16 else (1 / 16, 1 / 8)  # the GPU cases' grids at K = 576
    g = torch.Generator().manual_seed(0)
    x = dyadic((1, 64, 9, 10), -4, 4, sx, g)
    w = dyadic((32, 64, 3, 3), -2, 2, sw, g)
    b = dyadic((32,), -2, 2, 1 / 16, g)
    z = F.conv2d(x, w, b, 1, 1)
    assert torch.equal(F.conv2d(x.float(), w.float(), b.float(), 1, 1).double(), z)  # fp32 holds every sum
    rounded, ties = rounding_stats(z, tdt)
    assert rounded >= 0.10 and ties >= 0.01
    ref = rne(z, tdt)

    def mismatches(got):
        return int((got.view(torch.int16) != ref.view(torch.int16)).sum())

    assert mismatches(z.to(tdt)) == 0 and not elt_ulps(z.to(tdt), ref, tdt).any()
    lo, hi = elt_neighbours(z, tdt)
    assert bool((lo <= z).all() and (z <= hi).all() and ((lo == hi) == (ref.double() == z)).all())
    # (a) truncation toward zero: wrong wherever RNE rounds away from zero
    trunc = torch.where(z >= 0, lo, hi).to(tdt)
    n_a = mismatches(trunc)
    assert n_a >= 0.05 * z.numel() and int(elt_ulps(trunc, ref, tdt).abs().max()) == 1
    # (b) round-half-away: wrong on the ties whose even neighbour is the one nearer zero
    tie = (lo != hi) & ((z - lo) == (hi - z))
    away = torch.where(tie, torch.where(z >= 0, hi, lo), ref.double()).to(tdt)
    n_b = mismatches(away)
    assert 0 < n_b <= int(tie.sum()) and n_b >= 0.25 * int(tie.sum())
    assert bool((elt_ulps(away, ref, tdt) != 0)[~tie].sum() == 0)
    # (c) one term of magnitude 1/16 dropped from one output whose neighbours are at most 1/16 apart
    #     (|z| < 16 in bf16; any output in fp16, whose sums stay far below 2^7): that element is reported
    idx = next(i for i in (z.abs() < 16).nonzero().tolist())
    dropped = z.clone()
    dropped[tuple(idx)] -= 1 / 16
    got_c = dropped.to(tdt)
    assert mismatches(got_c) == 1 and elt_ulps(got_c, ref, tdt)[tuple(idx)] != 0
    #     and the same term (one tap of one input channel, |x w| = 1/16) dropped by every output pixel
    xs, ws = x.clone(), w.clone()
    xs[:, 5], ws[:, 5, 1, 1] = 1 / 4, 1 / 4
    z_all = F.conv2d(xs, ws, b, 1, 1)
    ws[:, 5, 1, 1] = 0
    z_drop = F.conv2d(xs, ws, b, 1, 1)
    assert torch.equal(z_all - z_drop, torch.full_like(z_all, 1 / 16))
    assert int((z_drop.to(tdt).view(torch.int16) != rne(z_all, tdt).view(torch.int16)).sum()) >= 0.3 * z.numel()
    # (d) leaky slope 0.1 (computed in fp32, as an epilogue would) where the reference uses 0.125
    ref_d = rne(torch.where(z > 0, z, z * 0.125), tdt)
    zf = z.float()
    got_d = torch.where(zf > 0, zf, zf * 0.1).to(tdt)
    neg = z < 0
    bad_d = got_d.view(torch.int16) != ref_d.view(torch.int16)
    assert int(bad_d[neg].sum()) >= 0.9 * int(neg.sum()) and not bad_d[~neg].any()


def test_exact_comparator_bites_e4m3():
    """The comparator of tests/test_gpu_fp8_exact.py (whole byte buffers against torch's e4m3fn cast of the
    clamped float64 reference) on one of its cases (tile 35, cin 64, 3x3, act none, both output scales):
    it must report each of (a) truncation toward zero, (b) round-half-away, (c) a store without the clamp
    (past 448 the cast gives the NaN code, which helpers.elt_ulps never accepts as a neighbour),
    (d) subnormals flushed to zero and (e) dq read one channel off -- and nothing on the correct bytes."""
    import torch
    from ycx import _lib  # noqa: F401 -- first: a missing library fails this test, it does not skip it
    import test_gpu_fp8_exact as T
    from helpers import E4M3, e4m3_is_nan, elt_neighbours, elt_ulps
    o = T.operands(2, 13, 11, 64, 3, 1, 64)
    ref = o.z.permute(0, 2, 3, 1).contiguous()  # act none, all 64 channels, NHWC
    so_hi, so_lo, _ = T.out_scales(ref, "comparator")

    def rejected(got_bytes, so):
        try:
            T.assert_bytes(T.framed(got_bytes), T.framed(T.q8(ref, so)), "wrong store")
        except AssertionError:
            return int((got_bytes != T.q8(ref, so)).sum())
        return 0

    for so in (so_hi, so_lo):
        assert rejected(T.q8(ref, so), so) == 0
        v = (ref * so).clamp(-448, 448)
        lo, hi = elt_neighbours(v, E4M3)
        tie = (lo != hi) & ((v - lo) == (hi - v))
        trunc = torch.where(v >= 0, lo, hi).to(E4M3).view(torch.uint8)                              # (a)
        assert rejected(trunc, so) >= 0.05 * v.numel()
        away = torch.where(tie, torch.where(v >= 0, hi, lo), T.q8(ref, so).view(E4M3).double())     # (b)
        n_b = rejected(away.to(E4M3).view(torch.uint8), so)
        assert 0.25 * int(tie.sum()) <= n_b <= int(tie.sum())
    unclamped = (ref * so_hi).to(E4M3)                                                              # (c)
    n_nan = int(e4m3_is_nan(unclamped).sum())
    assert n_nan > 0 and rejected(unclamped.view(torch.uint8), so_hi) == n_nan
    d = elt_ulps(unclamped, T.q8(ref, so_hi).view(E4M3), E4M3)
    assert int(d.abs().max()) > 1 and bool((d.abs() > 1)[e4m3_is_nan(unclamped)].all())  # no NaN is "one code away"
    ok = T.q8(ref, so_lo)                                                                           # (d)
    flushed = torch.where((ok & 0x78) == 0, ok & 0x80, ok)
    n_sub = int(((ok & 0x78) == 0).sum() - ((ok & 0x7F) == 0).sum())
    assert n_sub > 0 and rejected(flushed, so_lo) == n_sub
    dq = 1.0 / (o.s_w * T.S_X)                                                                       # (e)
    acc = (ref - o.b) / dq                       # the accumulator, exact
    off = acc * dq.roll(-1) + o.b                # dq[co + 1] in place of dq[co]
    for so in (so_hi, so_lo):
        assert rejected(T.q8(off, so), so) >= 0.5 * ref.numel()
