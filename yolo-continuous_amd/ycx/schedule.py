"""Which kernel launches run a plan: a pure function of the lowered graph (``engine.Plan``), the
precision and four flags. Nothing here needs a device or the native library; ``Engine`` binds
the result to memory, one op per launch.

The decisions: the stem -> 3x3/s2 pair as one ycx_stem_conv2; the SPPCSPC k5 pools as one
cascaded ycx_maxpool; MP's k2 s2 pool folded into the 1x1 that reads it (``in_pool``); the 160^2
1x1 -> 1x1 pair (ycx_conv2d_pair); and that pair plus the MP branch's pooled 1x1
(ycx_conv2d_pair_pool). ``Schedule.launches`` lists the launches in graph order,
``Schedule.activation_bufs`` the buffers they need in allocation order.

A/B switches, read when a Schedule is built: YCX_NO_CONV_PAIR, YCX_NO_POOL_FUSE and
YCX_NO_POOL_CASCADE turn the pair (and with it the trio), the pool fold and the cascade off.
"""
import os

from ._lib import OUT_NCHW_F32, OUT_NHWC

ITEMSIZE = {'bf16': 2, 'fp16': 2, 'f32': 4, 'fp8': 1}


class Launch:
    """One kernel launch and the graph nodes it covers, by ``kind``:

    stem2      nodes (stem, conv)
    conv_pair  nodes (a, b) or (a, b, c, pool): a -> b, and c on the k2 s2 pool of a's map;
               ``store_a``: a's map is written
    conv       nodes (conv,) or (conv, pool), the pool folded into the conv (kinds conv, stem, stem_reorg)
    gconv      nodes (gconv,)
    deconv     nodes (deconv,)
    ghost      nodes (ghost,)
    depth      nodes (depth,): one ycx_space_depth move (Contract, Expand, Focus on an activation)
    classify   nodes (classify,): one ycx_classify (global average pool + the Classify head's dense layer)
    pool       nodes: the cascade's pools, ``levels`` of them
    copy       nodes (up | concat | tonchw,): ``src`` -> channels from ``off`` of ``dst``, upsampled
               by ``scale`` (1 or 2), ``nchw``: to the fp32 NCHW output
    """
    __slots__ = ('kind', 'nodes', 'store_a', 'levels', 'src', 'dst', 'off', 'scale', 'nchw')

    def __init__(self, kind, nodes, store_a=False, levels=1, src=None, dst=None, off=0, scale=1, nchw=False):
        self.kind, self.nodes, self.store_a, self.levels = kind, tuple(nodes), store_a, levels
        self.src, self.dst, self.off, self.scale, self.nchw = src, dst, off, scale, nchw


def cout_pad(precision, cout, stem=False):
    """Rows of a conv's packed weights: cout rounded up to what the kernels' tiles take."""
    if precision == 'f32' or (precision == 'fp8' and not stem):
        return -(-cout // 64) * 64
    if cout <= 32:
        return 32
    if cout <= 64:
        return 64
    return -(-cout // 128) * 128


def cascade_fits(h, w, c, esz):
    """Whether ycx_maxpool's one-launch cascade (levels > 1) takes an (h, w) map of c
    channels of esz bytes: it keeps two copies of the H x W plane of one channel
    slice (a 16-byte multiple dividing c, at most 128 channels) in 64 KB of LDS
    (ycx_misc.hip, ycx_maxpool). Mirrors the launcher's slice search exactly."""
    t = 128
    while t * esz >= 16:
        if c % t == 0 and 2 * h * w * t * esz <= 65536:
            return True
        t >>= 1
    return False


def stem2_pairs(nodes):
    """Stem -> 3x3/s2 conv pairs that run as one ycx_stem_conv2 (the stem map stays in LDS;
    16-bit and fp8 plans): the stem's output read by that conv only. Returns {id(stem): conv}."""
    pairs = {}
    for nd in nodes:
        if nd.kind != 'stem':
            continue
        v, p = nd.out, nd.p
        if v.role != 'act' or len(v.consumers) != 1 or v.buf is None or v.buf.c != v.c:
            continue
        c = v.consumers[0]
        q = c.p
        if c.kind != 'conv' or c.inputs[0] is not v or q['residual'] is not None or q['layout'] != OUT_NHWC:
            continue
        if not (p['k'] == 3 and p['p'] == 1 and p['s'] in (1, 2) and int(p['w'].shape[1]) == 3 and
                int(p['w'].shape[0]) == 32 and p['layout'] == OUT_NHWC):
            continue
        if not (q['k'] == 3 and q['s'] == 2 and q['p'] == 1 and int(q['w'].shape[0]) <= 64 and
                int(q['w'].shape[0]) % 8 == 0 and q['ho'] % 4 == 0 and q['wo'] % 32 == 0):
            continue
        if p['act'] != q['act']:  # the fused kernel is instantiated per (act, act) with both equal
            continue
        pairs[id(nd)] = c
    return pairs


def pool_cascades(nodes, esz):
    """Chains of 'same' stride-1 pools (the SPPCSPC k5 cascade, ``engine.pyramid``), each pool
    reading the previous one's output, written to adjacent slices of one buffer: run as
    one ycx_maxpool launch with levels = chain length (16-bit / fp8 plans, HIP_CASCADE
    kernel), when the map's plane fits the kernel's LDS (``cascade_fits``; larger maps,
    e.g. the stride-32 map of a 1472^2 input, keep one launch per pool).
    Returns {id(first pool): [pool nodes]}."""
    out, used = {}, set()

    def same_pool(nd):
        p = nd.p
        return nd.kind == 'pool' and p['s'] == 1 and p['k'] % 2 == 1 and p['p'] == p['k'] // 2

    for i, a in enumerate(nodes):
        if id(a) in used or not same_pool(a) or a.out.role in ('input', 'output'):
            continue
        if not cascade_fits(a.inputs[0].h, a.inputs[0].w, a.inputs[0].c, esz):
            continue
        chain = [a]
        for b in nodes[i + 1:]:
            prev = chain[-1]
            if not (same_pool(b) and b.p['k'] == a.p['k'] and b.inputs[0] is prev.out and
                    b.out.buf is a.out.buf and b.out.coff == prev.out.coff + prev.out.c and
                    b.out.role not in ('input', 'output')):
                break
            chain.append(b)
        if len(chain) > 1:
            out[id(a)] = chain
            used.update(id(nd) for nd in chain)
    return out


def pool_convs(nodes, precision):
    """MP's k2 s2 pools (nets/common.py:25-31) whose map is read only by one 1x1 / s1
    conv: the conv pools its operand while staging it (ycx_conv_desc.in_pool, 16-bit
    plans, and fp8 plans where cin % 128 == 0), so the pooled map is never written.
    yolov7: all five MP pools. Returns {id(conv node): pool node}."""
    fp8 = precision == 'fp8'
    out = {}
    for nd in nodes:
        if nd.kind != 'pool':
            continue
        p, x, v = nd.p, nd.inputs[0], nd.out
        if not (p['k'] == 2 and p['s'] == 2 and p['p'] == 0 and x.h == 2 * v.h and x.w == 2 * v.w):
            continue
        if x.role != 'act' or v.role != 'act' or len(v.consumers) != 1 or x.coff % 8 or x.buf.c % 8:
            continue
        c = v.consumers[0]
        q = c.p
        if c.kind != 'conv' or c.inputs[0] is not v or not (q['k'] == 1 and q['s'] == 1 and q['p'] == 0):
            continue
        cin, cout = int(q['w'].shape[1]), int(q['w'].shape[0])
        if cin % (128 if fp8 else 64) or cout_pad(precision, cout) % 64 or q['layout'] == OUT_NCHW_F32:
            continue
        if x.n * x.h * x.w * x.buf.c * (1 if fp8 else 2) >= (1 << 31) - 64:
            continue
        out[id(c)] = nd
    return out


def conv_pairs(nodes, precision, pooled):
    """1x1 -> 1x1 chains that run as one ycx_conv2d_pair launch (tile 55; 16-bit plans): a 1x1 / s1
    conv with cin 64 / 128 / 256 and 256 output channels on a map large enough for the
    weight-resident kernel (>= 8 64-pixel tiles per CU), whose output a second 1x1 / s1
    conv (cin 256, cout_pad 128 / 256) reads directly; the first conv's output is still
    stored when anything else reads it (yolov7: layer 11 -> layer 14 at 160^2, layer 11
    also feeding the MP branch). Returns {id(first conv): second conv}."""
    out, taken = {}, set()

    def pointwise(nd):
        q = nd.p
        return (nd.kind == 'conv' and q['k'] == 1 and q['s'] == 1 and q['p'] == 0 and q['residual'] is None and
                q['layout'] == OUT_NHWC and id(nd) not in pooled)

    for a in nodes:
        if not pointwise(a) or id(a) in taken:
            continue
        x, v = a.inputs[0], a.out
        cin, cout = int(a.p['w'].shape[1]), int(a.p['w'].shape[0])
        if cin not in (64, 128, 256) or cout != 256 or v.role != 'act' or v.buf is None:
            continue
        if x.n * x.h * x.w < 8 * 64 * 256 or (x.role != 'input' and (x.coff % 8 or x.buf.c % 8)):
            continue
        if len(v.consumers) > 1 and (v.coff % 8 or v.buf.c % 8):  # y1 is stored: ycx_conv2d_pair's 16-B stores
            continue
        for b in v.consumers:
            if not pointwise(b) or b.inputs[0] is not v or id(b) in taken or id(b) in out:
                continue
            cb = int(b.p['w'].shape[0])
            if cout_pad(precision, cb) not in (128, 256) or cb % 8:
                continue
            if b.out.role == 'act' and (b.out.coff % 8 or b.out.buf.c % 8):
                continue
            out[id(a)] = b
            taken.update((id(a), id(b)))
            break
    return out


def pair_pools(nodes, precision, pairs, pooled):
    """Pairs (``conv_pairs``) that also run the MP branch's 1x1 (ycx_conv2d_pair_pool): the
    first conv's only other reader is a k2 s2 max-pool already folded into its 1x1 conv c
    (``pool_convs``), c is 256 -> cout_pad 128 with an NHWC output on 8-channel bounds, and the
    map is h even, w % 32 == 0 (yolov7: layer 11 -> 14 with 12 -> 13). The 256-channel map is then
    neither stored nor read back. Returns {id(first conv): (pooled conv c, its pool node)}."""
    out = {}
    by_pool = {id(pl): c for c, pl in ((c, pooled[id(c)]) for c in nodes if id(c) in pooled)}
    for a in nodes:
        b = pairs.get(id(a))
        if b is None:
            continue
        v = a.out
        rest = [nd for nd in v.consumers if nd is not b]
        if len(rest) != 1 or id(rest[0]) not in by_pool or v.role != 'act' or v.h % 2 or v.w % 32:
            continue
        c = by_pool[id(rest[0])]
        q, cc = c.p, int(c.p['w'].shape[0])
        if int(q['w'].shape[1]) != 256 or cout_pad(precision, cc) != 128 or cc % 8 or q['residual'] is not None:
            continue
        if q['layout'] != OUT_NHWC or c.out.role != 'act' or c.out.coff % 8 or c.out.buf.c % 8:
            continue
        out[id(a)] = (c, rest[0])
    return out


class Schedule:
    """The launches of a plan in one precision, and the activation buffers they need.

    fuse_pool=False: every pool writes its map; fuse_pair=False: every 1x1 of a pair stores its
    map (fp8 calibration reads them all); fuse_pair_pool=False: a pair stores its first map for
    the MP branch's pooled 1x1."""

    def __init__(self, plan, precision, fuse_stem2=True, fuse_pool=True, fuse_pair=True, fuse_pair_pool=True):
        nodes, off = plan.graph.nodes, os.environ.get
        h16, low = precision in ('bf16', 'fp16'), precision != 'f32'  # low: the 16-bit and fp8 plans
        stem2 = stem2_pairs(nodes) if low and fuse_stem2 else {}
        cascades = pool_cascades(nodes, ITEMSIZE[precision]) if low and not off('YCX_NO_POOL_CASCADE') else {}
        # each pass leaves alone what the one before it took: pooled -> pairs -> trios
        pooled = pool_convs(nodes, precision) if low and fuse_pool and not off('YCX_NO_POOL_FUSE') else {}
        pairs = conv_pairs(nodes, precision, pooled) if h16 and fuse_pair and not off('YCX_NO_CONV_PAIR') else {}
        trios = pair_pools(nodes, precision, pairs, pooled) if fuse_pair_pool else {}

        groups = (stem2.values(), pooled.values(), pairs.values(), (c for c, _ in trios.values()),
                  *(chain[1:] for chain in cascades.values()))
        inside = {id(nd) for group in groups for nd in group}  # nodes that run in another node's launch
        self.launches = []

        def add(kind, *covered, **kw):
            self.launches.append(Launch(kind, covered, **kw))

        for nd in nodes:
            i, k = id(nd), nd.kind
            if i in inside:
                continue
            if i in stem2:
                add('stem2', nd, stem2[i])
            elif i in pairs:
                trio = trios.get(i, ())
                add('conv_pair', nd, pairs[i], *trio, store_a=len(nd.out.consumers) > 1 and not trio)
            elif k in ('conv', 'stem', 'stem_reorg'):
                add('conv', nd, *([pooled[i]] if i in pooled else []))
            elif k in ('gconv', 'deconv', 'ghost', 'depth', 'classify'):
                add(k, nd)
            elif k == 'pool':
                chain = cascades.get(i, [nd])
                add('pool', *chain, levels=len(chain))
            elif k == 'up':  # an unfused upsample may write a slice of a concat buffer
                add('copy', nd, src=nd.inputs[0], dst=nd.out, off=nd.out.coff, scale=2)
            elif k == 'concat':
                for v, coff in nd.p['copies']:
                    add('copy', nd, src=v, dst=nd.out, off=coff)
            elif k == 'tonchw':
                add('copy', nd, src=nd.inputs[0], dst=nd.out, nchw=True)
            else:
                raise AssertionError(k)

        # in order of first use (fp8 calibration keys its amax list on it); a stem2 pair's stem map stays in LDS
        in_lds = {id(nd.out) for nd in nodes if id(nd) in stem2}
        self.activation_bufs, seen = [], set()
        for nd in nodes:
            for v in [nd.out] + nd.inputs:
                b = v.buf
                if b is not None and id(b) not in seen and id(v) not in in_lds:
                    seen.add(id(b))
                    self.activation_bufs.append(b)
