"""ycx_ibin_decode: the tolerance yardstick and the bandwidth (probe; nothing here is asserted).

    python tests/probes/ibin_bench.py tol   [results.json]
    python tests/probes/ibin_bench.py bench [results.json]

tol: on the shapes of tests/test_gpu_ibin_decode.py (5 x 7, 9 x 8, 20 x 20; na 1, 3; nc 1, 3, 80; n 2; N(0, 2)
logits, that file's seeds) the existing ycx_idetect_decode against oracle.ref_post.idetect_eval, as
max |gpu - ref| / max |ref| over the whole z tensor: the figure IDETECT_REL_ERR of the test file is the
largest of these. The IDetect head of a case is the IBin head's x, y, w-regression, h-regression,
objectness and class logits, so both kernels see the same numbers. Next to it the same measure for
ycx_ibin_decode against the test file's torch restatement, per column class, with the share of rows its
near-tie rule leaves out.

bench: the decode at the workload's shape (640 x 640, bs 32, nc 80, na 3, levels 80 / 40 / 20): one launch
per level, three launches timed together, against the bytes the kernel must move (the head read once, z and
xview written once), and ycx_idetect_decode at the matching shape (no 85) as the yardstick. Device events
around ITERS rounds of the three launches after a warm-up; the two arms alternate, REPS measurements each;
medians with lowest and highest."""
import ctypes
import json
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.join(HERE, "..", "..")
for p in (os.path.join(HERE, ".."), REPO, os.path.join(REPO, "yolo-continuous_amd")):
    sys.path.insert(0, p)
from ycx import _lib as L  # noqa: E402

ITERS, REPS = 50, 10
BS, NA, NC, LEVELS, STRIDES = 32, 3, 80, (80, 40, 20), (8.0, 16.0, 32.0)
ANCHORS3 = [[12, 16, 19, 36, 40, 28], [36, 75, 76, 55, 72, 146], [142, 110, 192, 243, 459, 401]]


def tol(out):
    import test_gpu_ibin_decode as T
    from helpers import rel_err
    from oracle import ref_post
    dev = torch.device("cuda:0")
    bins = T.bin_centres()
    lines = []
    for h, w in T.SHAPES:
        for na in (1, 3):
            for nc in (1, 3, 80):
                no = nc + 3 + 2 * T.GROUP
                head = T.random_head(h, w, na, nc, seed=1000 + 100 * h + 10 * na + nc)
                x5 = head.view(T.N, na, no, h, w)
                same = torch.cat([x5[:, :, 0:3], x5[:, :, 2 + T.GROUP:3 + T.GROUP], x5[:, :, 2 + 2 * T.GROUP:]], 2)
                same = same.reshape(T.N, na * (nc + 5), h, w).contiguous()
                zi = T.run_idetect(dev, same, na, 8.0)
                zr, _ = ref_post.idetect_eval([same], [T.ANCHORS[:2 * na]], na, nc + 5, [8.0])
                line = dict(h=h, w=w, na=na, nc=nc, no=no, idetect_rel_err=rel_err(zi, zr),
                            idetect_xy=rel_err(zi[..., :2], zr[..., :2]), idetect_wh=rel_err(zi[..., 2:4], zr[..., 2:4]),
                            idetect_conf=rel_err(zi[..., 4:], zr[..., 4:]))
                z_ref, _, p = T.ibin_level_ref(head, T.ANCHORS, na, 8.0, bins, bins)
                z_all, _ = T.run_ibin(dev, head, na, 8.0, bins, bins)
                z = z_all[:, T.ROW_OFF:T.ROW_OFF + na * h * w]
                skip = T.near_tie(p)
                got, ref = z.reshape(-1, nc + 5), z_ref.reshape(-1, nc + 5)
                errs = T.col_err(got, ref)
                wh = [float(T.col_err(got[~skip[:, j], 2 + j:3 + j], ref[~skip[:, j], 2 + j:3 + j])[0]) for j in (0, 1)]
                line.update(ibin_xy=float(errs[:2].max()), ibin_wh=max(wh), ibin_wh_all_rows=float(errs[2:4].max()),
                            ibin_conf=float(errs[4:].max()), ibin_whole_z=rel_err(z, z_ref),
                            skipped_rows=int(skip.any(1).sum()), rows=int(skip.shape[0]))
                print(json.dumps(line), flush=True)
                lines.append(line)
    top = dict(idetect_rel_err_max=max(v['idetect_rel_err'] for v in lines),
               ibin_col_err_max=max(max(v['ibin_xy'], v['ibin_wh'], v['ibin_conf']) for v in lines),
               skipped_rows=sum(v['skipped_rows'] for v in lines), rows=sum(v['rows'] for v in lines))
    print(json.dumps(top), flush=True)
    if out:
        with open(out, 'w') as f:
            json.dump(dict(summary=top, cases=lines), f, indent=1)


def level_desc(i, no, rows, off):
    d = L.DecodeDesc()
    d.n, d.h, d.w, d.na, d.no, d.rows_total, d.row_off = BS, LEVELS[i], LEVELS[i], NA, no, rows, off
    for a in range(2 * NA):
        d.anchors_scaled[a] = float(ANCHORS3[i][a])
    return d


def bench(out):
    import test_gpu_ibin_decode as T
    dev = torch.device("cuda:0")
    st = L.stream_handle(dev)
    rows = sum(NA * s * s for s in LEVELS)
    bins = (ctypes.c_float * T.BINS)(*T.bin_centres().tolist())
    arms, moved, keep = {}, {}, []
    for name, no, nz in (('ibin', NC + 3 + 2 * T.GROUP, NC + 5), ('idetect', NC + 5, NC + 5)):
        heads = [torch.randn(BS, NA * no, s, s, device=dev) * 2.0 for s in LEVELS]
        z = torch.empty(BS, rows, nz, device=dev)
        xvs = [torch.empty(BS, NA, s, s, no, device=dev) for s in LEVELS]
        descs, off = [], 0
        for i, s in enumerate(LEVELS):
            descs.append(level_desc(i, no, rows, off))
            off += NA * s * s
        keep += [heads, z, xvs, descs]
        moved[name] = 4 * BS * rows * (no + nz + no)  # head read once, z and xview written once

        def call(name=name, heads=heads, z=z, xvs=xvs, descs=descs):
            for i in range(len(LEVELS)):
                if name == 'ibin':
                    rc = L.lib.ycx_ibin_decode(ctypes.byref(descs[i]), ctypes.c_float(STRIDES[i]), T.BINS, bins, bins,
                                               heads[i].data_ptr(), z.data_ptr(), xvs[i].data_ptr(), st)
                else:
                    rc = L.lib.ycx_idetect_decode(ctypes.byref(descs[i]), ctypes.c_float(STRIDES[i]),
                                                  heads[i].data_ptr(), z.data_ptr(), xvs[i].data_ptr(), st)
                L.check(rc, name)
        arms[name] = call

    def once(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ITERS):
            call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / ITERS

    for call in arms.values():
        for _ in range(3):
            call()
    torch.cuda.synchronize()
    t = {k: [] for k in arms}
    for _ in range(REPS):
        for k, call in arms.items():
            t[k].append(once(call))
    line = dict(bs=BS, image=640, nc=NC, na=NA, levels=list(LEVELS), iters=ITERS, reps=REPS)
    for k in arms:
        med = statistics.median(t[k])
        line[f"{k}_ms"] = round(med, 4)
        line[f"{k}_lo_hi"] = [round(min(t[k]), 4), round(max(t[k]), 4)]
        line[f"{k}_bytes"] = moved[k]
        line[f"{k}_gb_per_s"] = round(moved[k] / med / 1e6, 1)
    line['ibin_bw_over_idetect_bw'] = round(line['ibin_gb_per_s'] / line['idetect_gb_per_s'], 3)
    line['idetect_spread'] = round((max(t['idetect']) - min(t['idetect'])) / statistics.median(t['idetect']), 3)
    print(json.dumps(line), flush=True)
    if out:
        with open(out, 'w') as f:
            json.dump(line, f, indent=1)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else 'bench'
    {'tol': tol, 'bench': bench}[mode](sys.argv[2] if len(sys.argv) > 2 else None)
