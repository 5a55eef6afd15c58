"""The cases of the schedule fixture (tests/golden/g7_schedule.json) and its compact form, shared by
tests/test_schedule.py and tests/golden/make_golden_schedule.py.

A schedule depends on the graph's shapes only, never on weight values, so the networks keep their
constructor weights. A node is named by its index in ``plan.graph.nodes``:

  ["stem2", stem, conv]   ["conv_pair", a, b, c|-1, pool|-1, store_a]   ["conv", node, pool|-1]
  ["gconv", node]   ["pool", first, levels]   ["copy", src producer|-1, node, off, scale, nchw]

and a buffer is [n, h, w, c]."""
import functools

import grouped_case
import p6_case
from helpers import ANCHORS
from ycx.engine import Plan
from ycx.nets.yolo import Model
from ycx.utils.helper_io import cvt_cfg

NETS = {'yolov7': lambda: Model(cvt_cfg('yolov7'), ANCHORS, 80),
        'yolov7-tiny': lambda: Model(cvt_cfg('yolov7-tiny'), ANCHORS, 1),
        'p6-mini': lambda: Model(p6_case.p6_mini(), p6_case.ANCHORS4, p6_case.NC),
        'gx-mini': lambda: Model(grouped_case.gx_mini(), grouped_case.ANCHORS2, grouped_case.NC)}
SHAPES = [('yolov7', (1, 3, 640, 640)), ('yolov7', (2, 3, 640, 640)),  # below the pair's pixel threshold
          ('yolov7', (8, 3, 640, 640)),     # pair and trio; the flag and environment variations run here
          ('yolov7', (32, 3, 640, 640)),
          ('yolov7', (8, 3, 640, 608)),     # the 160 x 152 map fails w % 32: pair, no trio
          ('yolov7', (1, 3, 1472, 1472)),   # cascade_fits false: three k5 pools
          ('yolov7-tiny', (2, 3, 640, 640)), ('yolov7-tiny', (8, 3, 640, 640)),
          ('p6-mini', p6_case.SHAPE), ('p6-mini', (8,) + p6_case.SHAPE[1:]),  # stem_reorg, DownC's pooled 1x1
          ('gx-mini', grouped_case.SHAPE)]  # gconv launches, an unfused upsample
PRECISIONS = ('bf16', 'fp16', 'f32', 'fp8')
FLAGS = ('fuse_stem2', 'fuse_pool', 'fuse_pair', 'fuse_pair_pool')
ENV = ('YCX_NO_CONV_PAIR', 'YCX_NO_POOL_FUSE', 'YCX_NO_POOL_CASCADE')
VARIED = ('yolov7', (8, 3, 640, 640))


def cases():
    """{case id: (net, shape, precision, flags switched off, environment switch set or None)}, grouped
    by (net, shape) so that a run in this order builds every plan once."""
    out = {}
    for net, shape in SHAPES:
        base = f"{net}-{shape[0]}x{shape[2]}x{shape[3]}"
        for prec in PRECISIONS:
            if net == 'gx-mini' and prec == 'fp8':  # check_plan_precision refuses grouped convs in fp8
                continue
            out[f"{base}-{prec}"] = (net, shape, prec, (), None)
        if (net, shape) == VARIED:
            for prec in ('bf16', 'fp8'):
                for off in [(f,) for f in FLAGS] + [('fuse_pool', 'fuse_pair')]:  # the last: the calibration engine
                    out[f"{base}-{prec}-no-{'-'.join(f[5:] for f in off)}"] = (net, shape, prec, off, None)
                for env in ENV:
                    out[f"{base}-{prec}-{env}"] = (net, shape, prec, (), env)
    return out


@functools.lru_cache(maxsize=2)  # a yolov7 plan holds its folded float64 weights
def plan(net, shape):
    return Plan(NETS[net](), shape)


def encode(plan, schedule):
    """(launches, buffers) of a Schedule in the fixture's compact form."""
    index = {id(nd): i for i, nd in enumerate(plan.graph.nodes)}

    def ix(nd):
        return index[id(nd)]

    def row(la):
        k, nd = la.kind, la.nodes
        if k == 'conv_pair':
            return [k, ix(nd[0]), ix(nd[1])] + ([ix(nd[2]), ix(nd[3])] if len(nd) > 2 else [-1, -1]) + [la.store_a]
        if k == 'conv':
            return [k, ix(nd[0]), ix(nd[1]) if len(nd) > 1 else -1]
        if k == 'pool':
            return [k, ix(nd[0]), la.levels]
        if k == 'copy':
            src = la.src.producer
            return [k, ix(src) if src is not None else -1, ix(nd[0]), la.off, la.scale, la.nchw]
        return [k] + [ix(n) for n in nd]

    return [row(la) for la in schedule.launches], [[b.n, b.h, b.w, b.c] for b in schedule.activation_bufs]
