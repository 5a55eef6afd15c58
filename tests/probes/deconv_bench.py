"""Time ycx_deconv2d and the wide-stride depthwise shapes of ycx_conv2d_grouped alone, at the layer sizes a
yolov7-width CSP path would give a RobustConv2: 128 -> 128 channels restoring an 80^2 map and 256 -> 256
restoring a 40^2 map, bs 32, bf16, s = 2, 4, 8 (probe; nothing here is asserted).

One JSON line per launch (ms; device events around ITERS back-to-back launches after a warm-up, the median
of REPS such measurements), each with its byte floor: the bytes the launch must move (input map, weights
and output map once) over the HBM rate, 8.0 TB/s peak and 6.29 TB/s as measured with a float4 copy.
  deconv   a  ycx_deconv2d;
           b  the unfused alternative it replaces, in the same process: the existing 1x1 conv
              (ycx_conv2d, the tile its picker takes) with N = s*s*cout output channels, which writes the
              [n][h][w][s*s*cout] intermediate, plus one ycx_copy_channels pass over that many bytes
              (the depth-to-space move; the library has no such kernel, a plain copy is its floor);
           and b / a, and the largest difference of a's output from b's 1x1 result put in place.
  dwconv   the depthwise (k 7, s 4) and (k 11, s 8) convs on the full-resolution map."""
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "yolo-continuous_amd"))
from ycx import _lib as L  # noqa: E402
from ycx.engine import pack_deconv_weights  # noqa: E402

ITERS, REPS, N = 50, 5, 32
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12  # bytes / s
SHAPES = [(80, 128), (40, 256)]       # (restored map, channels)


def timed(call):
    for _ in range(5):
        call()
    out = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ITERS):
            call()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / ITERS)
    return statistics.median(out)


def floors(nbytes):
    return dict(bytes=nbytes, floor_ms_8p0=round(nbytes / HBM_PEAK * 1e3, 4), floor_ms_6p29=round(nbytes / HBM_COPY * 1e3, 4))


def conv_desc(h, cin, cout, k, s, pad, ho, groups=0):
    d = L.ConvDesc()
    d.n, d.h, d.w, d.cin, d.in_c_off, d.in_c_stride = N, h, h, cin, 0, cin
    d.kh = d.kw = k
    d.stride, d.pad, d.ho, d.wo = s, pad, ho, ho
    d.cout, d.cout_pad, d.out_c_off, d.out_c_stride = cout, cout, 0, cout
    d.act, d.dtype, d.out_layout, d.groups = L.ACT_NONE, L.DT_BF16, L.OUT_NHWC, groups
    d.out_scale = d.res_scale = 1.0
    return d


def bench_deconv(dev, st, hw, C, s):
    h = hw // s
    x = torch.randn(N, h, h, C, device=dev).to(torch.bfloat16)
    w64 = torch.randn(C, C, s, s, dtype=torch.float64) * 0.1
    bias = torch.zeros(C, device=dev)
    y = torch.empty(N, hw, hw, C, device=dev, dtype=torch.bfloat16)
    wp = pack_deconv_weights(w64, torch.bfloat16).to(dev)
    dd = conv_desc(h, C, C, s, s, 0, hw)

    def run_a():
        L.check(L.lib.ycx_deconv2d(ctypes.byref(dd), x.data_ptr(), wp.data_ptr(), bias.data_ptr(), y.data_ptr(), st))
    ta = timed(run_a)

    R = s * s * C  # the same rows as a 1x1 conv's output channels: [R][1][1][cin]
    d1 = conv_desc(h, C, R, 1, 1, 0, h)
    bias_r = torch.zeros(R, device=dev)
    mid = torch.empty(N, h, h, R, device=dev, dtype=torch.bfloat16)
    mid2 = torch.empty_like(mid)
    cd = L.CopyDesc()
    cd.n, cd.h, cd.w, cd.c, cd.in_c_off, cd.in_c_stride = N, h, h, R, 0, R
    cd.out_c_off, cd.out_c_stride, cd.scale, cd.dtype, cd.out_layout, cd.dequant = 0, R, 1, L.DT_BF16, L.OUT_NHWC, 1.0

    def run_conv():
        L.check(L.lib.ycx_conv2d(ctypes.byref(d1), x.data_ptr(), wp.data_ptr(), bias_r.data_ptr(), mid.data_ptr(), None, st))

    def run_copy():
        L.check(L.lib.ycx_copy_channels(ctypes.byref(cd), mid.data_ptr(), mid2.data_ptr(), st))

    def run_b():
        run_conv()
        run_copy()
    nbytes = (x.numel() + wp.numel() + y.numel()) * 2
    base = dict(op='deconv', s=s, cin=C, cout=C, out_map=hw, bs=N, deconv_ms=round(ta, 4), **floors(nbytes),
                frac_of_floor_8p0=round(nbytes / HBM_PEAK * 1e3 / ta, 3))
    st1 = L.lib.ycx_conv2d(ctypes.byref(d1), x.data_ptr(), wp.data_ptr(), bias_r.data_ptr(), mid.data_ptr(), None, st)
    if st1 != L.YCX_OK:  # the dense kernels do not take this 1x1: there is no unfused alternative to time
        print(json.dumps(dict(base, unfused_ms=None, unfused_status=int(st1))), flush=True)
        return
    tconv, tcopy, tb = timed(run_conv), timed(run_copy), timed(run_b)
    want = mid.view(N, h, h, s, s, C).permute(0, 1, 3, 2, 4, 5).reshape(N, hw, hw, C)  # depth-to-space on the host side
    diff = float((y.float() - want.float()).abs().max())
    tile = L.lib.ycx_conv_tile_name(L.lib.ycx_conv_pick_tile(ctypes.byref(d1))).decode()
    print(json.dumps(dict(base, unfused_ms=round(tb, 4), unfused_conv1x1_ms=round(tconv, 4),
                          unfused_copy_ms=round(tcopy, 4), conv1x1_tile=tile, unfused_over_deconv=round(tb / ta, 2),
                          max_abs_diff_vs_conv1x1=diff)), flush=True)


def bench_dw(dev, st, hw, C, k, s):
    x = torch.randn(N, hw, hw, C, device=dev).to(torch.bfloat16)
    ho = (hw + 2 * (k // 2) - k) // s + 1
    y = torch.empty(N, ho, ho, C, device=dev, dtype=torch.bfloat16)
    wg = (torch.randn(k, k, C, 1) * 0.1).to(dev)
    bias = torch.zeros(C, device=dev)
    d = conv_desc(hw, C, C, k, s, k // 2, ho, groups=C)
    d.act = L.ACT_SILU

    def run():
        L.check(L.lib.ycx_conv2d_grouped(ctypes.byref(d), x.data_ptr(), wg.data_ptr(), bias.data_ptr(), y.data_ptr(),
                                         None, st))
    t = timed(run)
    nbytes = (x.numel() + y.numel()) * 2 + wg.numel() * 4
    print(json.dumps(dict(op='dwconv', k=k, s=s, c=C, in_map=hw, bs=N, dw_ms=round(t, 4), **floors(nbytes),
                          frac_of_floor_8p0=round(nbytes / HBM_PEAK * 1e3 / t, 3))), flush=True)


def main():
    dev = torch.device("cuda:0")
    st = L.stream_handle(dev)
    for hw, C in SHAPES:
        for s in (2, 4, 8):
            bench_deconv(dev, st, hw, C, s)
        for k, s in ((7, 4), (11, 8)):
            bench_dw(dev, st, hw, C, k, s)


if __name__ == "__main__":
    main()
