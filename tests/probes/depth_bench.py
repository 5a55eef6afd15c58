"""Time ycx_space_depth in each mode at the map sizes a 640 x 640 stem or neck sees, bs 32, bf16, gain 2
(probe; nothing here is asserted).

Rows (map, channels): (160, 64) and (80, 256). Four arms per row, ms per launch, device events around ITERS
back-to-back launches after a warm-up; the arms run interleaved, one measurement of each per round, REPS
rounds, and a row reports each arm's median and its lowest and highest measurement:
  contract  [n][h][w][c] -> [n][h/2][w/2][4c]
  focus     the same move in ReOrg's block order
  expand    [n][h][w][c] -> [n][2h][2w][c/4]
  copy      ycx_copy_channels of the same [n][h][w][c] map, dense to dense: the same bytes read and written,
            the yardstick.
Every arm reads and writes n*h*w*c elements. Ratios: arm / copy (1.0 = the copy's rate); ``copy_spread`` is
the copy arm's (highest - lowest) / median, the run-to-run spread the ratios are read against. Before the
timing each mode's output is compared with torch's own view / permute, bit for bit.

    python tests/probes/depth_bench.py [results.json]"""
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "yolo-continuous_amd"))
from ycx import _lib as L  # noqa: E402

ITERS, REPS, N, S = 20, 10, 32, 2
ROWS = [(160, 64), (80, 256)]


def once(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ITERS


def desc(mode, hw, c):
    d = L.DepthDesc()
    d.n, d.h, d.w, d.c, d.in_c_off, d.in_c_stride = N, hw, hw, c, 0, c
    if mode == L.SD_EXPAND:
        d.ho, d.wo, d.out_c_stride = hw * S, hw * S, c // (S * S)
    else:
        d.ho, d.wo, d.out_c_stride = hw // S, hw // S, c * S * S
    d.out_c_off, d.gain, d.mode, d.dtype = 0, S, mode, L.DT_BF16
    return d


def torch_move(mode, x):
    """The reference modules' forward (nets/common.py:767, 793-798, 807-812) on an NHWC tensor."""
    t = x.permute(0, 3, 1, 2)
    n, c, h, w = t.shape
    if mode == L.SD_CONTRACT:
        y = t.reshape(n, c, h // S, S, w // S, S).permute(0, 3, 5, 1, 2, 4).reshape(n, c * S * S, h // S, w // S)
    elif mode == L.SD_EXPAND:
        y = t.reshape(n, S, S, c // S ** 2, h, w).permute(0, 3, 4, 1, 5, 2).reshape(n, c // S ** 2, h * S, w * S)
    else:
        y = torch.cat([t[..., ::2, ::2], t[..., 1::2, ::2], t[..., ::2, 1::2], t[..., 1::2, 1::2]], 1)
    return y.permute(0, 2, 3, 1).contiguous()


def main():
    dev = torch.device("cuda:0")
    st = L.stream_handle(dev)
    lines = []
    for hw, c in ROWS:
        x = torch.randn(N, hw, hw, c, device=dev).to(torch.bfloat16)
        y = torch.empty_like(x).reshape(-1)  # every arm writes as many elements as it reads
        cd = L.CopyDesc()
        cd.n, cd.h, cd.w, cd.c, cd.in_c_off, cd.in_c_stride = N, hw, hw, c, 0, c
        cd.out_c_off, cd.out_c_stride, cd.scale, cd.dtype = 0, c, 1, L.DT_BF16
        cd.out_layout, cd.dequant = L.OUT_NHWC, 1.0
        descs = dict(contract=desc(L.SD_CONTRACT, hw, c), focus=desc(L.SD_FOCUS, hw, c),
                     expand=desc(L.SD_EXPAND, hw, c))

        def mover(d):
            return lambda: L.check(L.lib.ycx_space_depth(ctypes.byref(d), x.data_ptr(), y.data_ptr(), st))

        arms = {k: mover(d) for k, d in descs.items()}
        arms['copy'] = lambda: L.check(L.lib.ycx_copy_channels(ctypes.byref(cd), x.data_ptr(), y.data_ptr(), st))
        exact = {}
        for k, d in descs.items():
            arms[k]()
            torch.cuda.synchronize()
            exact[k] = bool(torch.equal(y.view(torch.int16), torch_move(d.mode, x).reshape(-1).view(torch.int16)))
        for call in arms.values():
            for _ in range(5):
                call()
        torch.cuda.synchronize()
        t = {k: [] for k in arms}
        for _ in range(REPS):
            for k, call in arms.items():
                t[k].append(once(call))
        med = {k: statistics.median(v) for k, v in t.items()}
        moved = 2 * N * hw * hw * c * 2  # bytes read + written, every arm
        line = dict(map=hw, c=c, bs=N, gain=S, dtype='bf16', iters=ITERS, reps=REPS, bytes_moved=moved)
        for k in arms:
            line[f"{k}_ms"] = round(med[k], 4)
            line[f"{k}_lo_hi"] = [round(min(t[k]), 4), round(max(t[k]), 4)]
            line[f"{k}_gb_per_s"] = round(moved / med[k] / 1e6, 1)
        for k in descs:
            line[f"{k}_over_copy"] = round(med[k] / med['copy'], 3)
        line.update(copy_spread=round((max(t['copy']) - min(t['copy'])) / med['copy'], 3), bit_exact=exact)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], 'w') as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
