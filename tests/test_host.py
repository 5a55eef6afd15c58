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


@pytest.mark.parametrize('dtype_name', ['bfloat16', 'float16'])
def test_framed_comparator_bites(dtype_name):
    """The framed whole-buffer comparison of tests/test_gpu_conv_exact.py (helpers: sentinel-filled buffer,
    slice in its interior, live padding rows) on a synthetic result. Each of these must fail it:
    (a) a padding channel stored after the slice, (b) a zero stored into the lead, (c) one unwritten
    element whose true value is 0, (d) an fp32 NCHW plane block written one plane late. And (a)-(c) pass
    the comparison the file used before -- a zero-filled buffer with the slice as its last channels and
    zero padding rows, where a stored padding channel is act(0) = 0 in the next pixel's lead: the gap the
    frame closes, shown without running a wrong kernel."""
    import torch
    from helpers import (OUT_LEAD, OUT_TAIL, SENTINEL, assert_bits, dyadic, expected_frame, expected_planes,
                         live_padding_share, out_frame, out_planes, rne)
    tdt = getattr(torch, dtype_name)
    n, h, w, cout, cpad = 2, 5, 3, 24, 32
    g = torch.Generator().manual_seed(1)
    z = dyadic((n, h, w, cpad), -8, 8, 1 / 16, g)  # NHWC "true sums" of all cpad channels, padding rows live
    z[1, 2, 1, 5] = 0.0                            # a true value of 0 does occur on these grids
    ref, pad = rne(z[..., :cout], tdt), rne(z[..., cout:], tdt)
    live_padding_share(pad, SENTINEL)

    def fails(got, exp):
        try:
            assert_bits(got, exp, "synthetic")
        except AssertionError:
            return True
        return False

    def old_frame(elems):  # the earlier convention: zeros, the slice at the end, nothing behind it
        buf = torch.zeros(n, h, w, OUT_LEAD + cout, dtype=tdt)
        buf[..., OUT_LEAD:] = elems
        return buf

    new_exp, old_exp = expected_frame(ref), old_frame(ref)
    assert not fails(expected_frame(ref), new_exp) and not fails(old_frame(ref), old_exp)
    # (a) the first padding channel stored too: in the new frame its live value lands on the tail; in the old
    #     one a zero row's act(0) = 0 lands on channel 0 of the next pixel's (zero) lead
    got = expected_frame(ref)
    got[..., OUT_LEAD + cout] = pad[..., 0]
    assert fails(got, new_exp)
    old = old_frame(ref).reshape(-1, OUT_LEAD + cout)
    old[1:, 0] = 0.0  # pixel p's spill is pixel p + 1's channel 0 (the last pixel's leaves the buffer)
    assert not fails(old.reshape(old_exp.shape), old_exp)
    # (b) a zero stored into the lead
    got = expected_frame(ref)
    got[0, 1, 2, 3] = 0.0
    assert fails(got, new_exp)
    old = old_frame(ref)
    old[0, 1, 2, 3] = 0.0
    assert not fails(old, old_exp)
    # (c) one element never written, its true value 0: the sentinel still stands there; a zero-filled buffer agrees
    got = expected_frame(ref)
    got[1, 2, 1, OUT_LEAD + 5] = SENTINEL
    assert fails(got, new_exp)
    old = old_frame(ref)
    old[1, 2, 1, OUT_LEAD + 5] = 0.0  # what torch.zeros left there
    assert not fails(old, old_exp)
    assert out_frame(n, h, w, cout, tdt).shape[3] == OUT_LEAD + cout + OUT_TAIL
    # (d) fp32 NCHW: every plane one plane late (out_c_off 2 where the descriptor says 1)
    r32 = z[..., :cout].permute(0, 3, 1, 2).float()
    late = out_planes(n, cout, h, w)  # [n][cout + 2][h][w]: the last plane lands on the trailing sentinel plane
    late[:, 2:cout + 2] = r32
    assert fails(late, expected_planes(r32)) and not fails(expected_planes(r32), expected_planes(r32))


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
