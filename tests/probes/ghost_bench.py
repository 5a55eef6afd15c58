"""Time ycx_ghost_dw on GhostConv's second half at the yolov7 640 map sizes, bs 32, bf16, SiLU (probe;
nothing here is asserted).

Rows (map, hidden channels c): (160, 32), (80, 64), (40, 128), (40, 512), (20, 256). Four arms per row, ms per
launch, device events around ITERS back-to-back launches after a warm-up; the arms run interleaved, one
measurement of each per round, REPS rounds, and a row reports each arm's median and its lowest and highest
measurement:
  a  ycx_ghost_dw in place: the hidden map is the first half of the 2c-wide buffer, only the second half is stored;
  b  ycx_ghost_dw out of place with a residual over all 2c channels (Ghost's shortcut);
  c  ycx_conv2d_grouped, the generic kernel, reading the first half and writing the second half of the same buffer;
  d  ycx_copy_channels from the first half to the second: the bytes arm a moves, the ceiling.
Ratios: a / c (below 1: the specialised kernel is faster) and d / a (1.0 = the copy's rate); b only against d."""
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "yolo-continuous_amd"))
from ycx import _lib as L  # noqa: E402

ITERS, REPS, N = 50, 5, 32
ROWS = [(160, 32), (80, 64), (40, 128), (40, 512), (20, 256)]


def once(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ITERS


def desc(hw, c, cout, in_off, in_stride, out_off, out_stride, res_stride=0):
    d = L.ConvDesc()
    d.n, d.h, d.w, d.cin, d.in_c_off, d.in_c_stride = N, hw, hw, c, in_off, in_stride
    d.kh = d.kw = 5
    d.stride, d.pad, d.ho, d.wo = 1, 2, hw, hw
    d.cout, d.cout_pad, d.out_c_off, d.out_c_stride = cout, cout, out_off, out_stride
    d.res_c_off, d.res_c_stride = 0, res_stride
    d.act, d.dtype, d.out_layout, d.groups = L.ACT_SILU, L.DT_BF16, L.OUT_NHWC, c
    d.out_scale = d.res_scale = 1.0
    return d


def main():
    dev = torch.device("cuda:0")
    st = L.stream_handle(dev)
    for hw, c in ROWS:
        buf = torch.randn(N, hw, hw, 2 * c, device=dev).to(torch.bfloat16)   # arms a, c, d: both halves of one buffer
        x = buf[..., :c].contiguous()                                        # arm b: the hidden map on its own
        res = torch.randn(N, hw, hw, 2 * c, device=dev).to(torch.bfloat16)
        yb = torch.empty_like(res)
        w = (torch.randn(5, 5, c, 1, dtype=torch.float64) * 0.1).float().to(dev)
        bias = torch.zeros(c, device=dev)
        da = desc(hw, c, 2 * c, 0, 2 * c, 0, 2 * c)
        db = desc(hw, c, 2 * c, 0, c, 0, 2 * c, res_stride=2 * c)
        dc = desc(hw, c, c, 0, 2 * c, c, 2 * c)
        cd = L.CopyDesc()
        cd.n, cd.h, cd.w, cd.c, cd.in_c_off, cd.in_c_stride = N, hw, hw, c, 0, 2 * c
        cd.out_c_off, cd.out_c_stride, cd.scale, cd.dtype, cd.out_layout, cd.dequant = c, 2 * c, 1, L.DT_BF16, L.OUT_NHWC, 1.0

        def run_a():
            L.check(L.lib.ycx_ghost_dw(ctypes.byref(da), buf.data_ptr(), w.data_ptr(), bias.data_ptr(), buf.data_ptr(),
                                       None, st))

        def run_b():
            L.check(L.lib.ycx_ghost_dw(ctypes.byref(db), x.data_ptr(), w.data_ptr(), bias.data_ptr(), yb.data_ptr(),
                                       res.data_ptr(), st))

        def run_c():
            L.check(L.lib.ycx_conv2d_grouped(ctypes.byref(dc), buf.data_ptr(), w.data_ptr(), bias.data_ptr(),
                                             buf.data_ptr(), None, st))

        def run_d():
            L.check(L.lib.ycx_copy_channels(ctypes.byref(cd), buf.data_ptr(), buf.data_ptr(), st))

        arms = dict(a=run_a, b=run_b, c=run_c, d=run_d)
        run_c()
        torch.cuda.synchronize()
        want = buf[..., c:].clone()
        run_a()
        torch.cuda.synchronize()
        same = bool(torch.equal(buf[..., c:], want))  # the two kernels' second halves, bit for bit
        for call in arms.values():
            for _ in range(5):
                call()
        t = {k: [] for k in arms}
        for _ in range(REPS):
            for k, call in arms.items():
                t[k].append(once(call))
        med = {k: statistics.median(v) for k, v in t.items()}
        moved = 2 * N * hw * hw * c * 2  # arm a: c channels read, c written
        line = dict(map=hw, c=c, bs=N)
        for k in arms:
            line[f"{k}_ms"] = round(med[k], 4)
            line[f"{k}_lo_hi"] = [round(min(t[k]), 4), round(max(t[k]), 4)]
        line.update(a_over_c=round(med['a'] / med['c'], 3), d_over_a=round(med['d'] / med['a'], 3),
                    d_over_b=round(2.5 * med['d'] / med['b'], 3),  # arm b moves 2.5x arm a's bytes (c + 2c read, 2c written)
                    a_gb_per_s=round(moved / med['a'] / 1e6, 1), a_equals_c_bits=same)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
