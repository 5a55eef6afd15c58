"""The cases of the packing fixture (tests/golden/g10_pack.json) and its compact form, shared by
tests/test_pack.py and tests/golden/make_golden_pack.py.

What an ``Engine`` packs and what its descriptors say needs no GPU: ``cpu_engine`` binds a plan to CPU
memory (``torch.empty`` never touches the activation pages) and runs the engine's own ``_build``. The
networks carry the seeded synthetic weights of the GPU tests, so the packed bytes are reproducible.

Per case ``encode`` gives {"ops": [[op kind, {descriptor name: [every field, in struct order]}, op_info,
[non-null pointer fields], [the p<i> that weight, weight2, weight3 point at]] ...], "packed": [[name, shape,
dtype, sha256 of the bytes (its first 12 hex digits)] ...], "conv_flops", "input_slots", "output_slots",
"workspace" (fp32 elements)}. Most rows recur from case to case (a precision changes few of them), so the file
keeps every distinct row once, in "table", and a case names its rows by their index there (``squeeze`` /
``expand``): an op is [kind, descriptors, op_info, pointers, weight names], a packed tensor [i of p<i>, row]."""
import ctypes
import functools
import hashlib
import json

import torch

import ghost_case
import grouped_case
import p6_case
import rc2_case
from helpers import make_model
from ycx import _lib as L
from ycx.engine import Engine, Plan
from ycx.nets.yolo import Model
from ycx.schedule import Schedule
from ycx.utils.synth import synthetic_state_dict


def _mini(cfg, anchors, nc, seed, state_dict=synthetic_state_dict):
    m = Model(cfg, anchors, nc).eval()
    m.load_state_dict(state_dict(m, seed=seed))
    return m


NETS = {'yolov7': lambda: make_model('yolov7', 80, 0)[0],
        'yolov7-tiny': lambda: make_model('yolov7-tiny', 1, 0)[0],
        'p6-mini': lambda: _mini(p6_case.p6_mini(), p6_case.ANCHORS4, p6_case.NC, p6_case.W_SEED),
        'gx-mini': lambda: _mini(grouped_case.gx_mini(), grouped_case.ANCHORS2, grouped_case.NC, grouped_case.W_SEED),
        'rc2-mini': lambda: _mini(rc2_case.rc2_mini(), rc2_case.ANCHORS2, rc2_case.NC, rc2_case.W_SEED,
                                  rc2_case.state_dict),
        'gh-mini': lambda: _mini(ghost_case.gh_mini(), ghost_case.ANCHORS2, ghost_case.NC, ghost_case.W_SEED)}
ALL = ('bf16', 'fp16', 'f32', 'fp8')
NO_FP8 = ('bf16', 'fp16', 'f32')  # check_plan_precision refuses gconv, deconv and ghost nodes in fp8
SHAPES = [('yolov7', (8, 3, 640, 640), ALL),       # stem pair, 1x1 pair and trio, pooled 1x1s, merged siblings,
                                                   # x2-upsample stores, NCHW heads
          ('yolov7-tiny', (2, 3, 640, 640), ALL),  # Leaky epilogues
          ('p6-mini', p6_case.SHAPE, ALL),         # stem_reorg
          ('gx-mini', grouped_case.SHAPE, NO_FP8),  # gconv with residual
          ('rc2-mini', rc2_case.SHAPE, NO_FP8),    # deconv
          ('gh-mini', ghost_case.SHAPE, NO_FP8)]   # ghost in place and with shortcut
# these also with engine._NO_SILU_PS set (SiLU convs packed plain): yolov7-tiny is Leaky throughout, so there the
# switch must change nothing; p6-mini's convs are SiLU
NO_SILU_PS = {'yolov7-tiny': ('bf16', 'fp8'), 'p6-mini': ('bf16', 'fp8')}
DTYPE = {'bf16': torch.bfloat16, 'f32': torch.float32, 'fp8': torch.float8_e4m3fn, 'fp16': torch.float16}
DT = {'bf16': L.DT_BF16, 'f32': L.DT_F32, 'fp8': L.DT_FP8, 'fp16': L.DT_F16}


def cases():
    """{case id: (net, shape, precision, engine._NO_SILU_PS)}, grouped by net so that a run in this order
    builds every plan once."""
    out = {}
    for net, shape, precisions in SHAPES:
        base = f"{net}-{shape[0]}x{shape[2]}x{shape[3]}"
        for prec in precisions:
            out[f"{base}-{prec}"] = (net, shape, prec, False)
        for prec in NO_SILU_PS.get(net, ()):
            out[f"{base}-{prec}-no-silu-ps"] = (net, shape, prec, True)
    return out


@functools.lru_cache(maxsize=2)  # a yolov7 plan holds its folded float64 weights
def plan(net, shape):
    return Plan(NETS[net](), shape)


def fp8_amax(bufs):
    """A synthetic calibration record for the buffers of ``Schedule.activation_bufs``: values over 13
    binades, every seventh 0.0 and every seventh inf (both take the scale-1.0 branch of
    ``Engine._assign_fp8_scales`` unless a finite positive member of their group outweighs the 0.0)."""
    def amax(i):
        if i % 7 == 3:
            return 0.0
        if i % 7 == 5:
            return float('inf')
        return 2.0 ** ((5 * i) % 13 - 6) * (1.0 + (i % 4) / 4.0)
    return [dict(c=b.c, amax=amax(i)) for i, b in enumerate(bufs)]


def cpu_engine(plan, precision, prepacked=None):
    """An Engine of the plan bound to CPU memory: everything ``Engine.__init__`` sets before ``_build``,
    with the CPU as the device (the constructor itself refuses one). Honours engine._NO_SILU_PS as set
    by the caller. prepacked: {'p<i>': tensor} to bind instead of packing."""
    e = Engine.__new__(Engine)
    e.plan, e.shape, e.device, e.precision = plan, plan.shape, torch.device('cpu'), precision
    e.dtype, e.dt = DTYPE[precision], DT[precision]
    e.schedule = Schedule(plan, precision)
    e.prepacked, e.graph_exec, e.scales = prepacked, None, {}
    e.graph, e.out_vals, e.is_list = plan.graph, plan.out_vals, plan.is_list
    if precision == 'fp8':
        amax = fp8_amax(e.schedule.activation_bufs)
        assert any(a['amax'] == 0.0 for a in amax) and any(a['amax'] == float('inf') for a in amax)
        e._assign_fp8_scales(amax)
    e._build()
    return e


def tensor_hash(t):
    return hashlib.sha256(t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()[:12]


def fields(d):
    return [getattr(d, name) for name, _ in d._fields_]


_CONV_OPS = (L.OP_CONV, L.OP_STEM, L.OP_STEM_REORG, L.OP_GCONV, L.OP_DECONV, L.OP_GHOST)
_POINTERS = [name for name, t in L.Op._fields_ if t is ctypes.c_void_p]


def encode(e):
    """An engine's ops, packed tensors and slots in the fixture's form (see the module docstring)."""
    name_of = {t.data_ptr(): k for k, t in e.packed.items()}
    assert len(name_of) == len(e.packed) and e.n_ops == len(e.op_info)
    ops = []
    for i in range(e.n_ops):
        op = e.ops[i]
        if op.kind in _CONV_OPS:
            descs = dict(conv=fields(op.d.conv))
        elif op.kind in (L.OP_STEM2, L.OP_CONV_PAIR):
            descs = dict(pair0=fields(op.d.pair[0]), pair1=fields(op.d.pair[1]), conv3=fields(op.conv3))
        elif op.kind == L.OP_POOL:
            descs = dict(pool=fields(op.d.pool))
        else:
            assert op.kind == L.OP_COPY
            descs = dict(copy=fields(op.d.copy))
        ops.append([op.kind, descs, e.op_info[i], [f for f in _POINTERS if getattr(op, f)],
                    [name_of.get(getattr(op, f)) for f in ('weight', 'weight2', 'weight3')]])
    assert [t.data_ptr() for t in e.params] == [t.data_ptr() for t in e.packed.values()]  # one order
    packed = [[k, list(t.shape), str(t.dtype), tensor_hash(t)] for k, t in e.packed.items()]
    return dict(ops=ops, packed=packed, conv_flops=e.conv_flops, input_slots=e.input_slots,
                output_slots=[e.output_slots.get(id(v), []) for v in e.out_vals],
                workspace=e.workspace.numel() if e.workspace is not None else 0)


def squeeze(enc, table):
    """A case of ``encode`` with its rows replaced by their index in ``table`` ({row as JSON: index}, extended
    here in order of first use)."""
    def ix(row):
        return table.setdefault(json.dumps(row, separators=(',', ':')), len(table))
    return dict(enc, ops=[[kind] + [ix(part) for part in parts] for kind, *parts in enc['ops']],
                packed=[[int(name[1:]), ix(row)] for name, *row in enc['packed']])


def expand(case, rows):
    """The inverse of ``squeeze``; rows: the file's "table" (a list)."""
    return dict(case, ops=[[kind] + [rows[i] for i in parts] for kind, *parts in case['ops']],
                packed=[[f"p{n}"] + rows[i] for n, i in case['packed']])
