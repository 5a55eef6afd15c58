"""Time ycx_classify at two head sizes, bs 32, bf16 (probe; nothing here is asserted).

Rows (map, channels, outputs): (20, 1024, 1000), a 1000-class head on a 640 x 640 input's stride-32 map, and
(20, 512, 80). Arms, ms per launch, device events around ITERS back-to-back launches after a warm-up; the arms
run interleaved, one measurement of each per round, REPS rounds, and a row reports each arm's median and its
lowest and highest measurement:
  classify    ycx_classify: the bf16 [n][h][w][c] map -> fp32 [n][cout] (two launches, one op)
  maxpool     ycx_maxpool k2 s2 of the same map: the in-project yardstick for a read-dominated kernel
  torch_f32   torch.mean(x, (1, 2), dtype=float32) + F.linear with the same fp32 weights: the same arithmetic
  torch_bf16  torch.mean(x, (1, 2)) + F.linear with bf16 weights: the pair as a bf16 torch model would run it
Bytes: classify's floor is input + weights + bias + output (the fp32 means it writes and reads back,
2 * n * c * 4, are on top and reported as ``classify_bytes_moved``); maxpool's is input + output. ``*_gb_per_s``
is floor bytes over the median time. ``classify_over_torch_*`` is classify / torch (below 1: classify is
faster); ``classify_spread`` is the classify arm's (highest - lowest) / median, the run-to-run spread the
ratios are read against. Before the timing the logits are compared with a float64 evaluation of the same
rounded inputs.

    python tests/probes/classify_bench.py [results.json]"""
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "yolo-continuous_amd"))
from ycx import _lib as L  # noqa: E402

ITERS, REPS, N = 50, 10, 32
ROWS = [(20, 1024, 1000), (20, 512, 80)]


def once(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ITERS


def main():
    dev = torch.device("cuda:0")
    st = L.stream_handle(dev)
    lines = []
    for hw, c, cout in ROWS:
        g = torch.Generator(device='cpu').manual_seed(hw + c + cout)
        x = torch.randn(N, hw, hw, c, generator=g).to(torch.bfloat16).to(dev)
        w = (torch.randn(cout, c, generator=g) / c ** 0.5).to(dev)
        b = (0.1 * torch.randn(cout, generator=g)).to(dev)
        w16, b16 = w.to(torch.bfloat16), b.to(torch.bfloat16)
        y = torch.empty(N, cout, device=dev)
        ws = torch.empty(N, c, device=dev)
        pooled = torch.empty(N, hw // 2, hw // 2, c, dtype=torch.bfloat16, device=dev)
        d = L.ClassifyDesc()
        d.n, d.h, d.w, d.c, d.in_c_off, d.in_c_stride, d.cout, d.dtype, d.dequant = N, hw, hw, c, 0, c, cout, L.DT_BF16, 1.0
        pd = L.PoolDesc()
        pd.n, pd.h, pd.w, pd.c, pd.in_c_off, pd.in_c_stride = N, hw, hw, c, 0, c
        pd.ho, pd.wo, pd.out_c_off, pd.out_c_stride = hw // 2, hw // 2, 0, c
        pd.k, pd.stride, pd.pad, pd.dtype, pd.levels = 2, 2, 0, L.DT_BF16, 1
        arms = dict(
            classify=lambda: L.check(L.lib.ycx_classify(ctypes.byref(d), x.data_ptr(), w.data_ptr(), b.data_ptr(),
                                                        y.data_ptr(), ws.data_ptr(), st)),
            maxpool=lambda: L.check(L.lib.ycx_maxpool(ctypes.byref(pd), x.data_ptr(), pooled.data_ptr(), st)),
            torch_f32=lambda: torch.nn.functional.linear(torch.mean(x, dim=(1, 2), dtype=torch.float32), w, b),
            torch_bf16=lambda: torch.nn.functional.linear(torch.mean(x, dim=(1, 2)), w16, b16))
        arms['classify']()
        torch.cuda.synchronize()
        ref = x.double().mean((1, 2)) @ w.double().t() + b.double()
        err = float((y.double() - ref).abs().max() / ref.abs().max())
        err_t = float((arms['torch_f32']().double() - ref).abs().max() / ref.abs().max())
        for call in arms.values():
            for _ in range(10):
                call()
        torch.cuda.synchronize()
        t = {k: [] for k in arms}
        for _ in range(REPS):
            for k, call in arms.items():
                t[k].append(once(call))
        med = {k: statistics.median(v) for k, v in t.items()}
        in_bytes = N * hw * hw * c * 2
        floor = in_bytes + 4 * (cout * c + cout + N * cout)
        pool_bytes = in_bytes + in_bytes // 4
        line = dict(map=hw, c=c, cout=cout, bs=N, dtype='bf16', iters=ITERS, reps=REPS, classify_floor_bytes=floor,
                    classify_bytes_moved=floor + 2 * N * c * 4, maxpool_bytes=pool_bytes,
                    classify_rel_err_vs_f64=err, torch_f32_rel_err_vs_f64=err_t)
        for k in arms:
            line[f"{k}_ms"] = round(med[k], 5)
            line[f"{k}_lo_hi"] = [round(min(t[k]), 5), round(max(t[k]), 5)]
        line.update(classify_gb_per_s=round(floor / med['classify'] / 1e6, 1),
                    classify_moved_over_floor=round((floor + 2 * N * c * 4) / floor, 4),
                    maxpool_gb_per_s=round(pool_bytes / med['maxpool'] / 1e6, 1),
                    classify_over_torch_f32=round(med['classify'] / med['torch_f32'], 3),
                    classify_over_torch_bf16=round(med['classify'] / med['torch_bf16'], 3),
                    classify_spread=round((max(t['classify']) - min(t['classify'])) / med['classify'], 3))
        print(json.dumps(line), flush=True)
        lines.append(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], 'w') as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
