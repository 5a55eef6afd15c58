"""The case table of tests/test_gpu_move_exact.py without a GPU: every pool, cascade and flat-fallback
case is built and its input conditions asserted from the float64 reference alone -- a border window
with a negative maximum and an inf among the outputs at every level, for the NaN variants between one
NaN output and half of all outputs NaN plus a window of NaN only -- then which kernel each flat case
lands on, the channel slice of every cascade, the patterns of the copy input with both its references,
and the NaN site of the fused-pool cases. Prints the ranges over the table (pytest -s)."""
import torch

from ycx import _lib as L  # first: without the library this test fails, it does not skip with the GPU file

import test_gpu_move_exact as T


def test_move_case_table_meets_its_conditions():
    shares, cases = [], 0

    def seen(o, what):
        nonlocal cases
        T.check_pool_conditions(o, what)
        cases += 1
        if o.nan:
            shares.extend(float(r.isnan().double().mean()) for r in o.ref)
            pos = o.x[..., o.in_off:o.in_off + o.c].isnan().double().mean()
            assert 0.005 <= float(pos) <= 0.02, f"{what}: NaN at {float(pos):.4f} of the positions"

    for dtype in T.DT_ALL:
        for k, s, p in T.KSP:
            for h, w in T.maps(s):
                for nan in T.nans(dtype):
                    seen(T.pool_case(dtype, T.N, h, w, T.C, k, s, p, 1, nan), f"pool k{k} s{s} {h}x{w} dtype {dtype}")
    for dtype in T.DT_FLOAT:
        for n, nan in [(2048, False), (2047, False), (2048, True)]:
            o = T.flat_case(dtype, n, nan)
            seen(o, f"flat n {n} dtype {dtype}")
            assert T.flat_side(o) == (n == 2048)
            assert o.x.numel() * o.x.element_size() <= (4 << 20) * (2 if dtype == L.DT_F32 else 1)
    for dtype in (L.DT_BF16, L.DT_F16, L.DT_FP8):
        for h, w, c, k in T.CASCADE_SHAPES:
            for levels in (2, 3):
                if dtype == L.DT_FP8 and c % 16:
                    assert T.cascade_slice(T.cascade_shell(dtype, h, w, c, k, levels)) == 0
                    continue
                for nan in T.nans(dtype):
                    o = T.cascade_case(dtype, h, w, c, k, levels, nan)
                    seen(o, f"cascade {h}x{w} c{c} k{k} levels {levels} dtype {dtype}")
                    assert T.cascade_slice(o) == {(11, 13, 48): 16, (7, 9, 16): 16, (20, 20, 136): 8,
                                                  (45, 45, 8): 8}[(h, w, c)]
    assert T.cascade_slice(T.cascade_shell(L.DT_BF16, 46, 46, 8, 3, 3)) == 0
    for dtype in T.DT_FLOAT:
        x = T.copy_input(dtype)  # asserts its patterns
        sl = x[..., T.IN_OFF:T.IN_OFF + T.COPY_SHAPE[3]]
        for scale in (1, 2):
            nhwc, nchw = T.copy_expected(dtype, scale, False), T.copy_expected(dtype, scale, True)
            # both references move the same pixels: the widened NHWC bits are the NCHW values
            a = T.widen(nhwc[..., T.OUT_OFF:T.OUT_OFF + sl.shape[3]].view(T.TDT[dtype])).permute(0, 3, 1, 2)
            b = nchw[:, 8:8 + sl.shape[3]].double()
            assert torch.equal(a.isnan(), b.isnan())
            assert torch.equal(T.bits(torch.where(a.isnan(), 0.0, a).float()), T.bits(torch.where(b.isnan(), 0.0, b).float()))
            assert bool(b.isnan().any()) and bool(((b == 0) & torch.signbit(b)).any())
    for n, h, w, cin, cout in T.F1_SHAPES:
        img, py, px = T.f1_nan_site(n, h, w)
        assert 0 <= img < n and 0 <= py < h and 0 <= px < w
    print(f"\n{cases} pool cases; NaN outputs {100 * min(shares):.2f}-{100 * max(shares):.2f} % per level")
