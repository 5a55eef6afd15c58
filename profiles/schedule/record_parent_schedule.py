"""Record tests/golden/g7_schedule.json from the fusion passes as Engine carried them at the parent
commit (66b2a91), before ycx.schedule existed. Kept as the record of how the fixture was made; it
cannot run on a tree that has ycx/schedule.py.

In an export of the parent commit (git archive 66b2a91 | tar -x -C <dir>), with this change's
tests/schedule_case.py and tests/golden/make_golden_schedule.py copied in (the case list and the
file writer; neither imports ycx.schedule at module level) and the built library in place:

    cd <dir> && python <this file> $(git -C <repository> rev-parse 66b2a91)

Drives the five passes the way tests/test_plan.py did then (Engine.__new__, then graph / dt / dtype
and the four flags), replays Engine._build's node ladder and writes the compact rows by hand: no
ycx.schedule and no schedule_case.encode()."""
import os
import sys

ROOT = os.getcwd()
sys.path.insert(0, os.path.join(ROOT, 'yolo-continuous_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
import make_golden_schedule as G  # noqa: E402
import schedule_case as C  # noqa: E402
import torch  # noqa: E402
from ycx import _lib as L  # noqa: E402
from ycx import engine  # noqa: E402

assert engine.__file__.startswith(ROOT), engine.__file__
assert not os.path.exists(os.path.join(ROOT, 'yolo-continuous_amd', 'ycx', 'schedule.py'))
DT = {'bf16': (L.DT_BF16, torch.bfloat16), 'f32': (L.DT_F32, torch.float32), 'fp8': (L.DT_FP8, torch.float8_e4m3fn),
      'fp16': (L.DT_F16, torch.float16)}


def record(net, shape, precision, off, env):
    for e in C.ENV:
        os.environ.pop(e, None)
    if env:
        os.environ[env] = '1'
    plan = C.plan(net, shape)
    eng = engine.Engine.__new__(engine.Engine)
    eng.graph = plan.graph
    eng.dt, eng.dtype = DT[precision]
    for f in C.FLAGS:
        setattr(eng, f, f not in off)
    nodes = plan.graph.nodes
    ix = {id(nd): i for i, nd in enumerate(nodes)}
    # ---- Engine._build at the parent, op emitters replaced by rows ----
    pairs = eng._stem2_pairs()
    fused = {id(c) for c in pairs.values()}
    bufs = [[b.n, b.h, b.w, b.c] for b in eng.activation_bufs()]
    cascades = eng._pool_cascades()
    for c in cascades.values():
        fused.update(id(nd) for nd in c[1:])
    pooled = eng._pool_convs()
    fused.update(id(nd) for nd in pooled.values())
    chains = eng._conv_pairs(pooled)
    fused.update(id(nd) for nd in chains.values())
    trios = eng._pair_pools(chains, pooled)
    fused.update(id(c) for c, _ in trios.values())
    rows = []

    def copy(x, node, off_, scale, nchw=False):
        rows.append(['copy', ix[id(x.producer)] if x.producer is not None else -1, ix[id(node)], off_, scale, nchw])

    for node in nodes:
        k = node.kind
        if id(node) in fused:
            continue
        if id(node) in pairs:
            rows.append(['stem2', ix[id(node)], ix[id(pairs[id(node)])]])
        elif id(node) in chains:
            a, b = node, chains[id(node)]
            c, pool = trios.get(id(node), (None, None))
            store_a = len(a.out.consumers) > 1 and c is None  # _pair_op
            rows.append(['conv_pair', ix[id(a)], ix[id(b)], ix[id(c)] if c is not None else -1,
                         ix[id(pool)] if pool is not None else -1, store_a])
        elif k in ('conv', 'stem', 'stem_reorg'):
            pool = pooled.get(id(node))
            rows.append(['conv', ix[id(node)], ix[id(pool)] if pool is not None else -1])
        elif k == 'gconv':
            rows.append(['gconv', ix[id(node)]])
        elif k == 'pool':
            rows.append(['pool', ix[id(node)], len(cascades.get(id(node), [node]))])
        elif k == 'up':
            copy(node.inputs[0], node, node.out.coff, 2)
        elif k == 'concat':
            for v, off_ in node.p['copies']:
                copy(v, node, off_, 1)
        elif k == 'tonchw':
            copy(node.inputs[0], node, 0, 1, True)
        else:
            raise AssertionError(k)
    os.environ.pop(env or '', None)
    return rows, bufs


if __name__ == '__main__':
    G.write(G.PATH, sys.argv[1], record)
