"""What every conv-kind node of a lowered graph (``engine.Plan``) hands its kernel: the packed weight and
bias tensors (the prepack file format, ``ycx.prepack``) and the ``ycx_conv_desc``. Pure functions of
(node, precision, a few explicit arguments): nothing here needs a device, an ``Engine``, an environment
variable or a module-level switch; ``Engine`` binds the results to memory.

Packed layouts (``spec``; bias fp32 [cout_pad] unless noted):

  conv                 [cout_pad][kh][kw][cin] in the activation dtype (the second conv of a stem pair:
                       16-bit whatever the plan, ``bf16_weights``)
  conv, fp8            e4m3 rows of w * s_w[co], [cout_pad][kh*kw*cin padded to 128 B]; bias [2 * cout_pad]:
                       the bias, then dq[co] = 1 / (s_w[co] s_x)
  stem, stem_reorg     [kh][kw][cin][cout_pad] fp32
  gconv, ghost         [kh][kw][cout][cin_g] fp32, bias [cout] (ghost: cout = the hidden width c, cin_g 1)
  deconv               [s*s][cout][cin] in the activation dtype, bias [cout]
  classify             [cout][c] fp32 in every precision: the centre tap of Classify's conv, bias [cout]

SiLU epilogues of the 16-bit / fp8 plans run on c' = -log2(e) c (YCX_ACT_SILU_PS): with ``silu_ps`` a dense
conv's weights and bias are scaled in float64 before their one rounding (fp8: the fp32 bias and dq rows,
so the e4m3 weights are unchanged). gconv, ghost, deconv and classify are never pre-scaled. A classify node
has no ycx_conv_desc (``desc`` is not for it): the engine fills its ycx_classify_desc."""
import torch

from . import _lib as L
from .schedule import cout_pad

CONV_KINDS = ('conv', 'stem', 'stem_reorg', 'gconv', 'deconv', 'ghost')
PACKED_KINDS = CONV_KINDS + ('classify',)  # every kind with packed tensors: the convs and the Classify head's dense layer
DENSE = ('conv', 'stem', 'stem_reorg')  # the kinds with padded output rows, a SiLU pre-scale and an fp8 path
DTYPE = {'bf16': torch.bfloat16, 'f32': torch.float32, 'fp8': torch.float8_e4m3fn, 'fp16': torch.float16}
DT = {'bf16': L.DT_BF16, 'f32': L.DT_F32, 'fp8': L.DT_FP8, 'fp16': L.DT_F16}


def conv_index(nodes):
    """{id(node): i} over the nodes with packed tensors (``PACKED_KINDS``) in graph order: node i packs into
    tensors p<2i>, p<2i+1>.
    Named by position in the graph, not by packing order: which convs fuse (stem pair, 1x1 pair) varies
    with the batch size and the A/B switches, and a prepack file is reused at any batch size."""
    return {id(nd): i for i, nd in enumerate(nd for nd in nodes if nd.kind in PACKED_KINDS)}


def pack_fp8_weights(wp):
    """float64 [cout_pad][cin][k][k] -> (e4m3 [cout_pad][ceil(k*k*cin / 128) * 128] as
    torch.float8_e4m3fn, float64 s_w[cout_pad]): per output channel the
    power-of-two scale that maps its max |w| into [224, 448], rows in
    [kh][kw][cin] order, zero-padded to whole 128-byte K steps (ycx.h)."""
    cpad = wp.shape[0]
    amax = wp.abs().amax(dim=(1, 2, 3))
    sw = torch.where(amax > 0, torch.exp2(torch.floor(torch.log2(448.0 / amax.clamp_min(1e-300)))),
                     torch.ones_like(amax))
    rows = (wp * sw.reshape(-1, 1, 1, 1)).permute(0, 2, 3, 1).reshape(cpad, -1)
    kt = rows.shape[1]
    ktp = -(-kt // 128) * 128
    out = torch.zeros((cpad, ktp), dtype=torch.float32)
    out[:, :kt] = rows.to(torch.float32)
    return out.clamp(-448.0, 448.0).to(torch.float8_e4m3fn), sw


def pack_deconv_weights(w64, dtype):
    """float64 [cin][cout][s][s] (torch's ConvTranspose2d layout) -> [s*s][cout][cin] in ``dtype``: the rows
    of ycx_deconv2d's GEMM, tap-major (tap = dy * s + dx), K = cin contiguous (include/ycx.h)."""
    cin, cout, s = int(w64.shape[0]), int(w64.shape[1]), int(w64.shape[2])
    return w64.permute(2, 3, 1, 0).reshape(s * s, cout, cin).contiguous().to(dtype)


def spec(node, precision, bf16_weights=False):
    """(weight shape, weight dtype, bias shape) of the node's packed tensors (the table above)."""
    k, (d0, d1) = node.p['k'], (int(s) for s in node.p['w'].shape[:2])
    if node.kind in ('gconv', 'ghost'):  # w [cout][cin_g][k][k]
        return (k, k, d0, d1), torch.float32, (d0,)
    if node.kind == 'deconv':            # w [cin][cout][s][s]
        return (k * k, d1, d0), DTYPE[precision], (d1,)
    if node.kind == 'classify':          # w [cout][c][1][1], the centre tap
        return (d0, d1), torch.float32, (d0,)
    stem = node.kind != 'conv'           # w [cout][cin][k][k]
    cpad = cout_pad(precision, d0, stem or bf16_weights)
    if stem:
        return (k, k, d1, cpad), torch.float32, (cpad,)
    if bf16_weights:
        return (cpad, k, k, d1), (torch.float16 if precision == 'fp16' else torch.bfloat16), (cpad,)
    if precision == 'fp8':
        return (cpad, -(-k * k * d1 // 128) * 128), torch.float8_e4m3fn, (2 * cpad,)
    return (cpad, k, k, d1), DTYPE[precision], (cpad,)


def pack(node, precision, *, bf16_weights=False, silu_ps, in_scale=1.0):
    """(weights, bias) of the node as CPU tensors of ``spec``'s shapes and dtypes, from the folded float64
    node.p['w'], node.p['b']. in_scale: the fp8 scale s_x of the buffer the node reads. A dense conv is
    zero-padded to cout_pad rows and pre-scaled (``silu_ps``) in float64, permuted, then rounded once."""
    w64, b64 = node.p['w'], node.p['b']
    assert node.kind in DENSE or not silu_ps
    if node.kind in ('gconv', 'ghost'):
        return w64.permute(2, 3, 0, 1).contiguous().to(torch.float32), b64.to(torch.float32)
    if node.kind == 'classify':
        return w64.reshape(w64.shape[0], w64.shape[1]).contiguous().to(torch.float32), b64.to(torch.float32)
    wshape, wdt, _ = spec(node, precision, bf16_weights)
    if node.kind == 'deconv':
        return pack_deconv_weights(w64, wdt), b64.to(torch.float32)
    stem = node.kind != 'conv'
    cout, cin, k = int(w64.shape[0]), int(w64.shape[1]), node.p['k']
    cpad = wshape[3] if stem else wshape[0]
    f8 = wdt == torch.float8_e4m3fn
    wp = torch.zeros((cpad, cin, k, k), dtype=torch.float64)
    wp[:cout] = w64
    bp = torch.zeros(cpad, dtype=torch.float64)
    bp[:cout] = b64
    ks = L.SILU_PS_K if silu_ps else 1.0
    if not f8:
        wp, bp = wp * ks, bp * ks
    if stem:
        wt = wp.permute(2, 3, 1, 0).contiguous().to(wdt)
    elif f8:
        wt, sw = pack_fp8_weights(wp)
        bp = torch.cat([bp * ks, ks / (sw * in_scale)])  # dq[co] = 1 / (s_w[co] s_x), both x ks
    else:
        wt = wp.permute(0, 2, 3, 1).contiguous().to(wdt)
    return wt, bp.to(torch.float32)


def take_prepacked(prepacked, i, spec):
    """Tensors p<i>, p<i+1> of a prepack file's {name: tensor}, checked against ``spec``."""
    wshape, wdt, bshape = spec
    wt, bt = prepacked.get(f"p{i}"), prepacked.get(f"p{i + 1}")
    if wt is None or bt is None or tuple(wt.shape) != wshape or wt.dtype != wdt or \
            tuple(bt.shape) != bshape or bt.dtype != torch.float32:
        raise ValueError(f"ycx: prepacked weights do not match this plan at tensor p{i}")
    return wt, bt


def scale_of(scales, v):
    """The fp8 scale of the buffer holding v ({id(buf): scale}; 1.0 where there is none)."""
    return scales.get(id(v.buf), 1.0) if v.buf is not None else 1.0


def desc(node, precision, *, bf16_weights=False, silu_ps, scales, pool=None):
    """The ycx_conv_desc of a conv-kind node (not a classify node), ``tile`` and ``k_split`` left 0 for the
    engine to pick.
    node.p carries kernel, stride, pad and groups for every kind (a deconv's k == s, a ghost's 5 / 1 / 2 and
    groups = c), the input and output values carry cin and cout (a ghost's c and 2c); what is left to tell
    apart is cout_pad, the input slice and the fp8 scales.
    scales: {id(buf): fp8 scale} (``Engine._assign_fp8_scales``; empty off fp8).
    pool: the k2 s2 pool node feeding this 1x1 conv, fused into it (``schedule.pool_convs``)."""
    p, x, out, r = node.p, node.inputs[0], node.out, node.p['residual']
    assert node.kind in DENSE or not silu_ps
    f8 = precision == 'fp8'
    d = L.ConvDesc()
    d.n, d.h, d.w, d.cin = x.n, x.h, x.w, x.c
    if x.role == 'input':
        d.in_c_off, d.in_c_stride = 0, x.c
    elif x.role == 'reorg':  # the image's own channel count; d.h, d.w, d.cin describe the reorganised map
        d.in_c_off, d.in_c_stride = 0, x.c // 4
    else:
        d.in_c_off, d.in_c_stride = x.coff, x.buf.c
    if pool is not None:  # read the pool's (2h, 2w) input map instead of its output
        src = pool.inputs[0]
        d.in_c_off, d.in_c_stride, d.in_pool = src.coff, src.buf.c, 1
    d.ho, d.wo, d.cout = p['ho'], p['wo'], out.c
    d.cout_pad = cout_pad(precision, out.c, node.kind != 'conv' or bf16_weights) if node.kind in DENSE else out.c
    d.kh = d.kw = p['k']
    d.stride, d.pad, d.act, d.leaky_slope = p['s'], p['p'], (L.ACT_SILU_PS if silu_ps else p['act']), p['slope']
    d.dtype, d.out_layout, d.groups = DT[precision], p['layout'], p.get('groups', 0)
    if p['layout'] == L.OUT_NCHW_F32:
        d.out_c_off, d.out_c_stride = 0, out.c
    else:
        d.out_c_off, d.out_c_stride = out.coff, out.buf.c
    if r is not None:
        d.res_c_off, d.res_c_stride = r.coff, r.buf.c
    d.out_scale = scale_of(scales, out) if (f8 and p['layout'] != L.OUT_NCHW_F32) else 1.0
    d.res_scale = 1.0 / scale_of(scales, r) if (f8 and r is not None) else 1.0
    return d


def flops(node):
    """Algorithmic FLOPs of a conv-kind node: 2*N*Ho*Wo*Cout*Cin*k*k (a grouped conv: Cin = cin_g, the
    second dim of its weights; a ghost node: its depthwise 5x5, 2*N*H*W*c*25); a transposed conv
    2*N*H*W*Cin*s*s*Cout: each input pixel feeds an s x s block (weights [cin][cout][s][s], k == s); a classify
    node: its dense layer, 2*N*Cout*C (k 1 on a 1 x 1 map)."""
    x, p = node.inputs[0], node.p
    px = x.h * x.w if node.kind == 'deconv' else p['ho'] * p['wo']
    return 2 * x.n * px * int(p['w'].shape[0]) * int(p['w'].shape[1]) * p['k'] ** 2


def conv_bytes(d, wt, isz, stem=False, pooled=False, residual=False, out_bytes=True):
    """Algorithmic HBM bytes of one conv launch (isz: the activation item size): its input map read once
    (the fp32 NCHW image for a stem -- a stem_reorg's 4C x h x w is the same C x 2h x 2w image --; the
    2x2-larger source map when an MP pool is fused in), the packed weights once, the residual once, the
    output written once (4x for the fused x2 upsample; fp32 for NCHW heads). The per-op roofline in
    bench.py prices each op against max(FLOP / MFMA peak, these bytes / HBM peak)."""
    px_in = d.n * d.h * d.w * (4 if pooled else 1)
    b = px_in * d.cin * (4 if stem else isz)
    b += wt.numel() * wt.element_size()
    px_out = d.n * d.ho * d.wo
    if residual:
        b += px_out * d.cout * isz
    if out_bytes:
        if d.out_layout == L.OUT_NCHW_F32:
            b += px_out * d.cout * 4
        else:
            b += px_out * d.cout * isz * (4 if d.out_layout == L.OUT_NHWC_UP2 else 1)
    return int(b)
