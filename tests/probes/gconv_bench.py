"""Time ycx_conv2d_grouped on depthwise and grouped layers at the yolov7 640 map sizes (160^2, 80^2,
40^2, 20^2 with 128 .. 1024 channels), bs 32, bf16 (probe; nothing here is asserted).

Per shape, one JSON line with three times (ms per layer; device events around ITERS back-to-back
launches after a warm-up, the median of REPS such measurements):
  a  the grouped kernel;
  b  the same layer through the dense ycx_conv2d, the only way the dense kernels can compute it:
     block-diagonal weights, one 64 -> 64 launch per 64-channel slice (the sum of the C / 64 launches);
  c  ycx_copy_channels over the input map, scaled by (input + output bytes) / (2 * input bytes) for
     a stride-2 layer (a copy reads and writes the same count): the bandwidth ceiling of moving the
     layer's activations once;
and a / c ("frac_of_copy" = c / a, 1.0 = the copy's rate) and b / a."""
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "yolo-continuous_amd"))
from ycx import _lib as L  # noqa: E402

ITERS, REPS, N = 50, 5, 32
# (map, channels, cin_g, k, s)
SHAPES = [(160, 128, 1, 3, 1), (160, 128, 1, 3, 2), (80, 256, 1, 3, 1), (80, 256, 1, 7, 1), (80, 256, 8, 3, 1),
          (40, 512, 1, 3, 1), (40, 512, 1, 5, 1), (40, 512, 4, 3, 1), (40, 512, 16, 3, 1), (20, 1024, 1, 3, 1),
          (20, 1024, 2, 3, 1), (20, 1024, 16, 3, 1)]


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


def desc(hw, c_in, c_out, k, s, in_off, in_stride, out_off, out_stride, groups):
    d = L.ConvDesc()
    d.n, d.h, d.w, d.cin, d.in_c_off, d.in_c_stride = N, hw, hw, c_in, in_off, in_stride
    d.kh = d.kw = k
    d.stride, d.pad = s, k // 2
    d.ho = d.wo = (hw + 2 * d.pad - k) // s + 1
    d.cout, d.cout_pad, d.out_c_off, d.out_c_stride = c_out, c_out, out_off, out_stride
    d.act, d.dtype, d.out_layout, d.groups = L.ACT_SILU, L.DT_BF16, L.OUT_NHWC, groups
    d.out_scale = d.res_scale = 1.0
    return d


def main():
    dev = torch.device("cuda:0")
    st = L.stream_handle(dev)
    for hw, C, g, k, s in SHAPES:
        x = torch.randn(N, hw, hw, C, device=dev).to(torch.bfloat16)
        ho = (hw + 2 * (k // 2) - k) // s + 1
        y = torch.empty(N, ho, ho, C, device=dev, dtype=torch.bfloat16)
        w64 = torch.randn(C, g, k, k, dtype=torch.float64) * 0.1
        bias = torch.zeros(C, device=dev)
        wg = w64.permute(2, 3, 0, 1).contiguous().float().to(dev)
        dg = desc(hw, C, C, k, s, 0, C, 0, C, C // g)

        def run_g():
            L.check(L.lib.ycx_conv2d_grouped(ctypes.byref(dg), x.data_ptr(), wg.data_ptr(), bias.data_ptr(),
                                             y.data_ptr(), None, st))
        ta = timed(run_g)
        ya = y.clone()

        # dense: per 64-channel slice a block-diagonal [64][k][k][64] weight
        dense = []
        for c0 in range(0, C, 64):
            wd = torch.zeros(64, 64, k, k, dtype=torch.float64)
            for co in range(64):
                gi = (co // g) * g
                wd[co, gi:gi + g] = w64[c0 + co]
            dd = desc(hw, 64, 64, k, s, c0, C, c0, C, 0)
            dense.append((dd, wd.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).to(dev)))

        def run_d():
            for dd, wd in dense:
                L.check(L.lib.ycx_conv2d(ctypes.byref(dd), x.data_ptr(), wd.data_ptr(), bias.data_ptr(), y.data_ptr(),
                                         None, st))
        tb = timed(run_d)
        # the two computations agree (bf16 weights on the dense side: a loose bar, this is a sanity check)
        diff = float((y.float() - ya.float()).abs().max()) / max(1e-9, float(ya.float().abs().max()))

        cd = L.CopyDesc()
        cd.n, cd.h, cd.w, cd.c, cd.in_c_off, cd.in_c_stride = N, hw, hw, C, 0, C
        cd.out_c_off, cd.out_c_stride, cd.scale, cd.dtype, cd.out_layout, cd.dequant = 0, C, 1, L.DT_BF16, L.OUT_NHWC, 1.0
        y2 = torch.empty_like(x)

        def run_c():
            L.check(L.lib.ycx_copy_channels(ctypes.byref(cd), x.data_ptr(), y2.data_ptr(), st))
        nbytes = (x.numel() + y.numel()) * 2
        tc = timed(run_c) * nbytes / (2 * x.numel() * 2)
        print(json.dumps(dict(map=hw, c=C, cin_g=g, k=k, s=s, bs=N, grouped_ms=round(ta, 4), dense_blockdiag_ms=round(tb, 4),
                              copy_ms=round(tc, 4), frac_of_copy=round(tc / ta, 3), dense_over_grouped=round(tb / ta, 2),
                              act_gb_per_s=round(nbytes / ta / 1e6, 1), dense_vs_grouped_rel_diff=round(diff, 4))),
              flush=True)


if __name__ == "__main__":
    main()
