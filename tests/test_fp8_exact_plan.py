"""The case table of tests/test_gpu_fp8_exact.py without a GPU: every input condition of every case,
from the float64 reference alone -- the e4m3 round trip and the span bound (asserted where the operands
are built), then per act the two output scales with their rounded, tie, saturated ([0.5 %, 20 %] at
so_hi) and subnormal (>= 0.1 % at so_lo) shares, the lossless fp32 cast of the fp32 NCHW cases, what each
tile-36 case reaches (tiles per block, ring wrap, store-counted waits: wres_plan), the 254
codes of the copy input, and the SiLU cases' excused cap. Prints the ranges over the table (pytest -s);
DESIGN.md §4 quotes them."""
import torch

from ycx import _lib as L  # first: without the library this test fails, it does not skip with the GPU file

import test_gpu_fp8_exact as T


def test_fp8_exact_case_table_meets_its_conditions():
    seen = []

    def scaled(ref, what):
        so_hi, so_lo, stats = T.out_scales(ref, what)
        assert so_hi / 512 <= so_lo <= so_hi / 64
        seen.append((what, so_hi, so_lo, stats[so_hi], stats[so_lo]))

    def conv(o, tile, cout, what, variant=None):
        for act, _, _, ref in T.conv_refs(o, cout, variant, tile):
            if variant == 'nchw_f32':
                assert torch.equal(ref.float().double(), ref)
            else:
                scaled(ref, f"{what} act {act}")

    for tile, cout, cpad in T.GENERAL:
        for cin, k, s in T.CKS:
            conv(T.operands(2, 13, 11, cin, k, s, cpad), tile, cout, f"tile {tile} cout {cout} cin {cin} k{k} s{s}")
    for tile in (34, 35):
        for variant in T.VARIANTS:
            o, cout = T.variant_case(tile, variant)
            conv(o, tile, cout, f"tile {tile} {variant}", variant)
    for h, w, cin, cout, cpad, plan in T.WRES:
        assert T.wres_plan(2 * h * w, cin, cout, cpad) == plan, (h, w, cin, cout, cpad)
        conv(T.operands(2, h, w, cin, 1, 1, cpad), 36, cout, f"tile 36 {h}x{w} cin {cin} cout {cout}")
    for h, w, cout in T.WS64:
        conv(T.operands(2, h, w, 64, 3, 1, 64), 37, cout, f"tile 37 {h}x{w} cout {cout}")
    for n, h, w, cin in T.HEADS:
        ref = T.operands(n, h, w, cin, 1, 1, 256).z[:, :255]
        assert torch.equal(ref.float().double(), ref)
    for h, w, cout in T.STEM_SHAPES:
        for s in (1, 2):
            for act, slope in T.ACTS:
                scaled(T.apply_act(T.stem_operands(h, w, cout, s).z, act, slope), f"stem {h}x{w} s{s} act {act}")
    for stem_s, cout, nhw, grid in T.STEM2_SHAPES:
        for act, slope in T.ACTS:
            scaled(T.stem2_operands(stem_s, cout, nhw, act, slope, grid)[5], f"stem2 s{stem_s} {grid} act {act}")
    T.copy_input()  # asserts the 254 finite codes inside the slice
    shares = []
    for tile, n, h, w, cin, k, s, cout, cpad in T.SILU_F8_CASES:
        o = T.silu_f8_operands(n, h, w, cin, k, s, cpad)
        for act in (L.ACT_SILU, L.ACT_SILU_PS):
            shares.append(T.silu_f8_conditions(o.z[:, :cout], o.b[:cout], act, f"tile {tile} act {act}")[3])
    for act in (L.ACT_SILU, L.ACT_SILU_PS):
        shares.append(T.stem2_silu_f8_conditions(act)[4])

    def rng(vals):
        return f"{100 * min(vals):.2f}-{100 * max(vals):.2f} %"

    print(f"\n{len(seen)} scaled references")
    print("rounded  so_hi", rng([s[3][0] for s in seen]), " so_lo", rng([s[4][0] for s in seen]))
    print("ties     so_hi", rng([s[3][1] for s in seen]), " so_lo", rng([s[4][1] for s in seen]))
    print("saturated at so_hi", rng([s[3][2] for s in seen]), " subnormal at so_lo", rng([s[4][3] for s in seen]))
    print("so_hi / so_lo", sorted({s[1] / s[2] for s in seen}), " SiLU excused", rng(shares))
