"""Time ycx_stem_conv_reorg at the P6 workload shape (1280^2 image, bs 8, 3 -> 64, stride 1; probe).

Prints one JSON line per precision: ms per call (device events over ITERS back-to-back calls after a
warm-up), the algorithmic HBM bytes (the fp32 image read once plus the output stored once; the 27 KB
of weights ignored) and the share of the HBM floor those bytes / 8 TB/s (spec) and / 6.3 TB/s (the
measured streaming rate) are of the time. The 6x6/s2 window re-reads the image from L2, not HBM."""
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "yolo-continuous_amd"))
from ycx import _lib as L  # noqa: E402

ITERS = 200


def main():
    dev = torch.device("cuda:0")
    n, h, w, cout = 8, 640, 640, 64  # the reorganised map of a 1280 x 1280 image
    x = torch.rand(n, 3, 2 * h, 2 * w, device=dev)
    wt = torch.randn(3, 3, 12, cout, device=dev) * 0.1
    b = torch.zeros(cout, device=dev)
    st = L.stream_handle(dev)
    for name, dt, tdt in (("bf16", L.DT_BF16, torch.bfloat16), ("fp16", L.DT_F16, torch.float16),
                          ("fp8", L.DT_FP8, torch.uint8), ("f32", L.DT_F32, torch.float32)):
        y = torch.empty(n, h, w, cout, device=dev, dtype=tdt)
        d = L.ConvDesc()
        d.n, d.h, d.w, d.cin, d.in_c_off, d.in_c_stride = n, h, w, 12, 0, 3
        d.ho, d.wo, d.cout, d.cout_pad, d.out_c_off, d.out_c_stride = h, w, cout, cout, 0, cout
        d.kh = d.kw = 3
        d.stride, d.pad, d.dtype, d.out_layout, d.out_scale = 1, 1, dt, L.OUT_NHWC, 1.0
        d.act = L.ACT_SILU if dt == L.DT_F32 else L.ACT_SILU_PS

        def call():
            L.check(L.lib.ycx_stem_conv_reorg(ctypes.byref(d), x.data_ptr(), wt.data_ptr(), b.data_ptr(),
                                              y.data_ptr(), st))
        iters = ITERS if dt != L.DT_F32 else 20
        for _ in range(10):
            call()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            call()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / iters
        nbytes = x.numel() * 4 + y.numel() * y.element_size()
        print(json.dumps(dict(kernel="ycx_stem_conv_reorg", precision=name, shape=[n, 3, 2 * h, 2 * w], cout=cout,
                              ms=round(ms, 4), hbm_bytes=nbytes, gb_per_s=round(nbytes / ms / 1e6, 1),
                              floor_share_8tbs=round(nbytes / 8.0e12 / (ms * 1e-3), 3),
                              floor_share_6p3tbs=round(nbytes / 6.3e12 / (ms * 1e-3), 3))), flush=True)


if __name__ == "__main__":
    main()
