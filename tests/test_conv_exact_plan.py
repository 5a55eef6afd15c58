"""Host-side (CPU) walk of the dense exact files' case tables: tests/test_gpu_conv_exact.py,
tests/trio_case.py / tests/test_gpu_conv_trio.py and tests/test_gpu_stem_reorg.py.

Every condition those files put on their inputs is a function of the float64 reference alone, so the
whole table is checked here without a GPU: the span bound and the lossless operands (asserted where
the operands are built), the >= 10 % rounded / >= 1 % tie shares of every 16-bit case, the lossless
fp32 cast of the fp32 cases, the SiLU cases' excused cap, the second-conv span of the pair and of
stem2, the live-padding share of every cout < cout_pad case (>= 90 % of what a padding channel would
store differs in its bits from the sentinel it would land on), the NaN guards' size and alignment, and
every descriptor the files build against the rules of the entry point it goes to, restated below from
include/ycx.h (not from the kernel source)."""
from ycx import _lib as L  # first: a missing library fails these tests, it does not skip them

import pytest
import torch
import torch.nn.functional as F

import test_gpu_conv_exact as E
import test_gpu_conv_trio as TT
import test_gpu_stem_reorg as R
import trio_case as TC
from helpers import (IN_LEAD, IN_TAIL, OUT_GUARD, OUT_TAIL, SENTINEL, SENTINEL_F32, guard_elems, live_padding_share,
                     rne, rounding_stats)

SIXTEEN = (L.DT_BF16, L.DT_F16)


# ---- include/ycx.h, restated ----
def interior(off, c, stride):
    """The frame: a slice with something in front of it and something behind it."""
    return 0 < off and off + c < stride


def conv_geometry_ok(d):
    return (d.ho == (d.h + 2 * d.pad - d.kh) // d.stride + 1 and d.wo == (d.w + 2 * d.pad - d.kw) // d.stride + 1
            and d.n > 0 and d.cout > 0 and d.cout_pad >= d.cout)


def check_conv2d_desc(d, residual=False):
    """ycx_conv_desc as ycx_conv2d / ycx_conv2d_ws take it (the struct's comment in ycx.h)."""
    assert conv_geometry_ok(d) and d.groups in (0, 1)
    vec = {L.DT_BF16: 8, L.DT_F16: 8, L.DT_F32: 4}[d.dtype]  # 16-byte vectors of input channels
    assert d.in_c_off % vec == 0 and d.in_c_stride % vec == 0 and d.in_c_stride % 8 == 0
    assert interior(d.in_c_off, d.cin, d.in_c_stride)
    if d.out_layout == L.OUT_NCHW_F32:  # planes: no channel-vector rule; one plane before, one after
        assert not residual and interior(d.out_c_off, d.cout, d.out_c_stride) and d.out_c_off == 1
    else:
        assert d.cout % 8 == 0 and d.out_c_off % 8 == 0 and d.out_c_stride % 8 == 0
        assert interior(d.out_c_off, d.cout, d.out_c_stride)
    if residual:
        assert d.res_c_off % 8 == 0 and d.res_c_stride % 8 == 0 and interior(d.res_c_off, d.cout, d.res_c_stride)
    if d.in_pool:  # 1x1 / s1 / p0, 16-bit with cin % 64 == 0
        assert d.in_pool == 1 and d.dtype in SIXTEEN and d.cin % 64 == 0
        assert (d.kh, d.kw, d.stride, d.pad) == (1, 1, 1, 0)
    if d.k_split > 1:  # 16-bit LDS-DMA tiles 16, 18, 56 only
        assert d.tile in (16, 18, 56) and d.dtype in SIXTEEN and not d.in_pool and d.out_layout != L.OUT_NCHW_F32
    if d.act == L.ACT_SILU_PS:
        assert d.dtype in SIXTEEN  # not the fp32 parity path


def check_input_guard(guard, pad, w, row_elems, itemsize):
    assert guard >= (pad * w + pad + 1) * row_elems and (guard * itemsize) % 16 == 0


def check_case(o, tile, cout, acts, what, cpad=None, layout=L.OUT_NHWC, lead=None, residual=None, k_splits=(0,),
               ref_of=None):
    """Conditions and descriptors of one ycx_conv2d case for each (act, slope) of ``acts``."""
    tdt = E.TDT[o.dtype]
    for act, slope in acts:
        ref = E.apply_act(o.z[:, :cout], act, slope)
        if residual is not None:
            ref = ref + residual.permute(0, 3, 1, 2)
        E.check_inputs(ref, torch.float32 if layout == L.OUT_NCHW_F32 else tdt, what)
        for ks in k_splits:
            kw = {} if lead is None else {'lead': lead}
            d = E.conv_desc(o, tile, cout, act, slope, residual=residual is not None, layout=layout, k_split=ks,
                            cpad=cpad, **kw)
            check_conv2d_desc(d, residual is not None)
            assert tuple(o.x_full.shape) == (d.n, d.h * (2 if d.in_pool else 1), d.w * (2 if d.in_pool else 1),
                                             d.in_c_stride)
            assert bool(o.x_full[..., :d.in_c_off].isnan().all()) and bool(o.x_full[..., d.in_c_off + d.cin:].isnan().all())
            assert not bool(o.x_full[..., d.in_c_off:d.in_c_off + d.cin].isnan().any())
            check_input_guard(E.input_guard(d, tdt.itemsize), d.pad, d.w * (2 if d.in_pool else 1), d.in_c_stride,
                              tdt.itemsize)
            if d.cout_pad > cout:
                E.check_live_padding(o, cout, d.cout_pad, act, slope, layout)
                wp, bp = E.packed(o, cout, d.cout_pad)
                assert wp.shape[0] == d.cout_pad and bool(wp[cout:].flatten(1).any(1).all())


def test_general_special_and_f32_cases():
    for tile, (cout, cin) in sorted(E.GENERAL.items()):
        for dtype in E.DT16:
            for k, s in E.KS:
                o = E.operands(dtype, *E.GENERAL_MAP, cin, k, s)
                check_case(o, tile, cout, E.ACTS, f"tile {tile} dtype {dtype} k{k} s{s}")
                assert E.cpad_of(cout, dtype) == cout
    for k, s in E.KS:
        check_case(E.f32_operands(k, s), 8, 64, E.ACTS, f"tile 8 k{k} s{s}")
    for tile, n, h, w, cin, cout, k, s in E.SPECIAL:
        for dtype in E.DT16:
            check_case(E.operands(dtype, n, h, w, cin, k, s, cout=cout), tile, cout, E.ACTS, f"tile {tile} {h}x{w}")


def test_epilogue_variant_and_below_pad_cases():
    n_live = 0
    for tile, variant in E.VARIANTS:
        for dtype in E.DT16:
            o, cout, cpad, layout, lead, r, ref = E.variant_case(tile, dtype, variant)
            what = f"tile {tile} dtype {dtype} {variant}"
            check_case(o, tile, cout, [E.VARIANT_ACT], what, cpad=cpad, layout=layout, lead=lead, residual=r)
            if r is not None:
                assert tuple(r.shape) == (o.n, o.ho, o.wo, cout)
            n_live += cpad is not None
            if variant in ('nchw_f32', 'cout_below_pad'):
                assert cpad > cout
    assert n_live == 2 * (5 + 7)  # nchw_f32 on five tiles, cout_below_pad on seven, both types
    tile, cout, cpad = E.UP2_BELOW_PAD
    for dtype in E.DT16:
        check_case(E.operands(dtype, *E.GENERAL_MAP, 64, 3, 1), tile, cout, [E.VARIANT_ACT], "up2 below pad", cpad=cpad,
                   layout=L.OUT_NHWC_UP2, lead=E.UP2_LEAD)
    for tile, h, w, cin, cout, cpad, k, s in E.BELOW_PAD:
        for dtype in E.DT16:
            check_case(E.operands(dtype, 2, h, w, cin, k, s), tile, cout, [E.BELOW_PAD_ACT], f"tile {tile} below pad",
                       cpad=cpad)
    for n, h, w, cout in E.KCM:
        for dtype in E.DT16:
            check_case(E.operands(dtype, n, h, w, 128, 3, 2), 16, cout, E.ACTS, f"KCM {h}x{w} cout {cout}")


def test_splitk_and_fused_pool_cases():
    for tile, cout in E.SPLITK_TILES:
        for cin, k, s in E.SPLITK_SHAPES:
            for dtype in E.DT16:
                o = E.operands(dtype, *E.GENERAL_MAP, cin, k, s)
                check_case(o, tile, cout, [E.SPLITK_ACT], f"split-K tile {tile} cin {cin}", k_splits=(0, 2, 3, 4))
                check_case(o, tile, cout, [E.SPLITK_ACT], f"split-K tile {tile} cin {cin} + residual",
                           residual=E.splitk_residual(o, cout), k_splits=(3,))
    for tile, cout, cin in E.POOL:
        for dtype in E.DT16:
            o = E.operands(dtype, *E.GENERAL_MAP, cin, 1, 1, pool=True)
            assert o.pool and tuple(o.x_full.shape[1:3]) == (2 * o.h, 2 * o.w)
            check_case(o, tile, cout, E.ACTS, f"in_pool tile {tile} cin {cin}")


def check_pair_descs(da, db):
    """ycx_conv2d_pair (ycx.h): a: cin 64 / 128 / 256 -> 256; b: 256 -> cout_pad 128 / 256, reads a's output."""
    for d in (da, db):
        assert (d.kh, d.kw, d.stride, d.pad, d.in_pool) == (1, 1, 1, 0, 0) and d.dtype in SIXTEEN
        assert d.out_layout == L.OUT_NHWC and d.out_c_off % 8 == 0 and d.out_c_stride % 8 == 0
        assert interior(d.out_c_off, d.cout, d.out_c_stride)
    assert da.cin in (64, 128, 256) and da.cout == 256 == da.cout_pad
    assert da.in_c_off % 8 == 0 and da.in_c_stride % 8 == 0 and interior(da.in_c_off, da.cin, da.in_c_stride)
    assert db.cin == 256 and db.cout_pad in (128, 256) and db.cout % 8 == 0 and db.cout <= db.cout_pad
    assert (db.in_c_off, db.in_c_stride) == (da.out_c_off, da.out_c_stride)
    assert (db.n, db.h, db.w) == (da.n, da.h, da.w) == (da.n, da.ho, da.wo)


def test_pair_cases():
    live = 0
    for cin, cout2, _ in E.PAIR:
        for dtype in E.DT16:
            tdt = E.TDT[dtype]
            c = E.pair_case(dtype, cin, cout2)  # asserts the second conv's span
            if dtype == L.DT_BF16:
                E.check_inputs(c.z1, tdt, "pair y1")
            E.check_inputs(c.z2, tdt, "pair y2")
            check_pair_descs(c.da, c.db)
            check_input_guard(E.input_guard(c.da, 2), 0, c.da.w, c.da.in_c_stride, 2)
            assert c.w2.shape[0] == c.cpad2 == c.db.cout_pad
            if c.cpad2 > cout2:
                live_padding_share(rne(c.z2_pad, tdt), SENTINEL)
                live += 1
    assert live == 2  # cout2 120 of 128, both types


def test_stem_and_stem2_cases():
    for h, w, cout in E.STEM_SHAPES:
        for s in (1, 2):
            c = E.stem_case(h, w, cout, s)  # asserts the span and the lossless operands
            for dtype in E.STEM_DTYPES:
                for act, slope in E.ACTS:
                    E.check_inputs(E.apply_act(c.z, act, slope), E.TDT[dtype], "stem")
                    d = E.stem_desc(c, dtype, act, slope)
                    # ycx_stem_conv: fp32 NCHW input with cin <= 4 channels, NHWC output as ycx_conv2d
                    assert conv_geometry_ok(d) and d.cin <= 4 and (d.in_c_off, d.in_c_stride) == (0, c.x.shape[1])
                    assert d.cout % 8 == 0 and d.out_c_off % 8 == 0 and d.out_c_stride % 8 == 0
                    assert interior(d.out_c_off, d.cout, d.out_c_stride) and d.cout_pad == d.cout
            check_input_guard(E.image_guard(1, w), 1, w, 1, 4)
    live = 0
    for stem_s, cout, nhw in E.STEM2:
        for act, slope in E.STEM2_ACTS:
            for dtype in E.DT16:
                tdt = E.TDT[dtype]
                c = E.stem2_case(dtype, stem_s, cout, nhw, act, slope)  # asserts the second conv's span
                if act == L.ACT_NONE and dtype == L.DT_BF16:
                    assert rounding_stats(c.z1, tdt)[0] >= E.MIN_ROUNDED
                E.check_inputs(c.ref, tdt, "stem2")
                ds, dc = E.stem2_descs(*nhw, dtype, stem_s, act, slope, cout)
                # ycx_stem_conv2: 3x3 / s 1 or 2 / pad 1, 3 -> 32, then 3x3 / s2 / pad 1, 32 -> cout (cout_pad 64)
                assert conv_geometry_ok(ds) and conv_geometry_ok(dc) and (dc.h, dc.w, dc.cin) == (ds.ho, ds.wo, ds.cout)
                assert (ds.kh, ds.pad, ds.cin, ds.cout) == (3, 1, 3, 32) and ds.stride in (1, 2)
                assert (dc.kh, dc.pad, dc.stride, dc.cout_pad) == (3, 1, 2, 64)
                assert dc.ho % 4 == 0 and dc.wo % 32 == 0 and ds.act == dc.act and ds.dtype == dc.dtype
                assert dc.cout % 8 == 0 and dc.out_c_off % 8 == 0 and dc.out_c_stride % 8 == 0
                assert interior(dc.out_c_off, dc.cout, dc.out_c_stride)
                assert tuple(c.ref.shape) == (nhw[0], cout, dc.ho, dc.wo) and c.wc.shape[0] == 64
                check_input_guard(E.image_guard(1, nhw[2]), 1, nhw[2], 1, 4)
                if cout < 64:
                    live_padding_share(rne(c.ref_pad, tdt), SENTINEL)
                    live += 1
    assert live == 4  # cout 48 of 64: two acts, two types


def test_head_cases():
    for n, h, w, cin in E.HEAD:
        for dtype in E.DT16:
            o = E.operands(dtype, n, h, w, cin, 1, 1)
            ref = o.z[:, :E.HEAD_COUT]
            E.check_inputs(ref, torch.float32)
            d, hd = E.head_descs(o)
            # ycx_conv2d_head: 1x1, act none, cout = na * no <= 256 padded to 256, fp32 NCHW heads without a stride
            assert conv_geometry_ok(d) and (d.kh, d.kw, d.stride, d.pad) == (1, 1, 1, 0) and d.act == L.ACT_NONE
            assert d.out_layout == L.OUT_NCHW_F32 and d.cout == hd.na * hd.no <= 256 == d.cout_pad and hd.no == hd.nc + 5
            assert d.in_c_off % 8 == 0 and d.in_c_stride % 8 == 0 and interior(d.in_c_off, d.cin, d.in_c_stride)
            assert hd.row_off + hd.na * d.ho * d.wo <= hd.rows_total and hd.conf_thres > 1.0
            check_input_guard(E.input_guard(d, 2), 0, w, d.in_c_stride, 2)
            assert OUT_GUARD >= h * w  # a plane written behind the last one stays inside the allocation
            live_padding_share(o.z[:, E.HEAD_COUT:256].float(), SENTINEL_F32)
            wp, _ = E.packed(o, E.HEAD_COUT, 256)
            assert bool(wp[E.HEAD_COUT:].flatten(1).any(1).all())


def test_silu_cases():
    for tile, n, h, w, cin, cout, k, s, k_split in E.SILU_CASES:
        for dtype in E.DT16:
            o = E.silu_operands(dtype, n, h, w, cin, k, s, cout)
            assert E.cpad_of(cout, dtype) == cout
            for act in E.SILU_ACTS:
                E.silu_conditions(o.z[:, :cout], act, E.TDT[dtype], f"tile {tile} dtype {dtype} act {act}")
                check_conv2d_desc(E.conv_desc(o, tile, cout, act, 0.0, k_split=k_split))
    for dtype in E.DT16:
        for act in E.SILU_ACTS:
            x, ws, bs, wc, bc, z2 = E.stem2_silu_operands(act, dtype)  # asserts the stem map off the boundaries
            E.silu_conditions(z2, act, E.TDT[dtype], "stem2 SiLU")
            assert wc.shape[0] == 64 and bool(wc.flatten(1).any(1).all())


def check_reorg_desc(d, o):
    """ycx_stem_conv_reorg (ycx.h): d is the conv after ReOrg; C = in_c_stride <= 4, in_c_off 0, cin 4C."""
    assert conv_geometry_ok(d) and 1 <= d.in_c_stride <= 4 and d.in_c_off == 0 and d.cin == 4 * d.in_c_stride
    assert (d.kh, d.kw, d.pad) == (3, 3, 1) and d.stride in (1, 2) and d.out_layout == L.OUT_NHWC
    assert d.cout_pad == 32 or d.cout_pad % 64 == 0
    assert d.cout % 8 == 0 and d.out_c_off % 8 == 0 and d.out_c_stride % 8 == 0
    assert interior(d.out_c_off, d.cout, d.out_c_stride) and d.out_c_stride == R.OUT_EXTRA + d.cout + OUT_TAIL
    assert tuple(o.x.shape) == (d.n, d.in_c_stride, 2 * d.h, 2 * d.w)
    g = R.image_guard(o)
    check_input_guard(g, 2, 2 * o.w, 1, 4)  # the 6x6 / pad-2 view; 16-byte aligned (the kernel asks for 8)


def test_stem_reorg_cases():
    def walk(o, dtype, cout, what, cpad=None):
        for act, slope in R.ACTS:
            R.check_inputs(R.apply_act(o.z[:, :cout], act, slope), R.TDT[dtype], what)
            d = R.desc_of(o, dtype, cout, act, slope, cpad)
            check_reorg_desc(d, o)
            wp, bp = R.packed(o, cout, d.cout_pad)
            assert wp.shape[3] == d.cout_pad == bp.shape[0]
            if d.cout_pad > cout:
                out_dt = R.TDT[dtype]
                live_padding_share(rne(R.apply_act(o.z[:, cout:d.cout_pad], act, slope), out_dt), SENTINEL)

    for h, w in R.SHAPES:
        for s in (1, 2):
            for cout in R.COUTS:
                for dtype in R.DTYPES:
                    walk(R.operands(h, w, s), dtype, cout, f"stem_reorg {h}x{w} s{s} cout {cout} dtype {dtype}")
    for dtype in R.DTYPES:
        cout, cpad = R.BELOW_PAD
        walk(R.operands(9, 11, 1), dtype, cout, "stem_reorg below pad", cpad=cpad)
        for s in (1, 2):
            walk(R.operands(9, 11, s, c=1), dtype, 32, "stem_reorg C1")
    for h, w, cout in R.FP8_CASES:
        for s in (1, 2):
            check_reorg_desc(R.desc_of(R.operands(h, w, s), L.DT_FP8, cout, out_scale=4.0), R.operands(h, w, s))
    assert R.SENTINEL_BYTE == 0x44  # e4m3 of 3.0
    for s in (1, 2):
        o = R.operands(9, 11, s, grid=R.SILU_GRID, seed=3)
        for dtype in (L.DT_BF16, L.DT_F16):
            for act in (L.ACT_SILU, L.ACT_SILU_PS):
                R.silu_conditions(o.z, act, R.TDT[dtype], "stem_reorg SiLU")
                check_reorg_desc(R.desc_of(o, dtype, 64, act), o)


def test_trio_cases():
    """ycx_conv2d_pair_pool (ycx.h): the pair's rules, plus c: in_pool 1 on (h / 2, w / 2), 256 -> cout_pad 128,
    cout % 8 == 0; a->h % 2 == 0, a->w % 32 == 0. The operands are random here, so the live-padding share
    comes from a float64 chain on the 16-bit operands."""
    live = 0
    for shape, cin, cout_b, cout_c, acts, _ in TT.CASES:
        for dtype in SIXTEEN:
            c = TC.TrioCase(None, dtype, shape, cin, cout_b, cout_c, acts)
            check_pair_descs(c.da, c.db)
            dc = c.dc
            assert dc.in_pool == 1 and (dc.h, dc.w) == (c.da.h // 2, c.da.w // 2) and c.da.h % 2 == 0 and c.da.w % 32 == 0
            assert dc.cin == 256 and dc.cout_pad == 128 and dc.cout % 8 == 0 and (dc.kh, dc.stride, dc.pad) == (1, 1, 0)
            assert dc.out_c_off % 8 == 0 and dc.out_c_stride % 8 == 0 and interior(dc.out_c_off, dc.cout, dc.out_c_stride)
            assert (dc.in_c_off, dc.in_c_stride) == (c.da.out_c_off, c.da.out_c_stride)  # the unfused launch reads ya
            x = c.host['x']
            assert tuple(x.shape) == (*shape, c.da.in_c_stride) and x.shape[3] == IN_LEAD + cin + IN_TAIL
            assert bool(x[..., :TC.X_OFF].isnan().all()) and bool(x[..., TC.X_OFF + cin:].isnan().all())
            assert not bool(x[..., TC.X_OFF:TC.X_OFF + cin].isnan().any())
            check_input_guard(c.x_guard, 0, shape[2], c.da.in_c_stride, 2)
            assert c.x_guard == guard_elems(0, shape[2], c.da.in_c_stride, 2)
            if cout_b == c.cpad_b and cout_c == 128:
                continue
            h = {k: v.double() for k, v in c.host.items()}
            xs = h['x'][..., TC.X_OFF:TC.X_OFF + cin]
            y1 = rne(TT._ref_act(xs @ h['wa'].T + h['ba'], acts[0]), c.tdt).double()
            if cout_b < c.cpad_b:
                live_padding_share(rne(TT._ref_act(y1 @ h['wb'][cout_b:].T + h['bb'][cout_b:], acts[1]), c.tdt), SENTINEL)
            if cout_c < 128:
                p = F.max_pool2d(y1.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
                live_padding_share(rne(TT._ref_act(p @ h['wc'][cout_c:].T + h['bc'][cout_c:], acts[2]), c.tdt), SENTINEL)
            live += 1
    assert live == 2 * 3  # cout 248 / 120 / 120 below their pads: three cases, both types
