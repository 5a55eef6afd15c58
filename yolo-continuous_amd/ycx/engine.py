"""Static execution plan of ``Model.forward`` on the HIP kernels.

Lowering (once per input shape / device / precision):

1. Walk ``model.model`` exactly like the reference interpreter loop
   (nets/yolo.py:143-153: ``m.f`` indexing into the per-layer outputs) and lower
   each module into graph nodes — conv (BN folded, RepConv re-parameterised,
   Bottleneck residual fused into the epilogue), stem conv (first conv on the
   fp32 NCHW image; ``stem_reorg`` when ReOrg precedes it: the space-to-depth is folded into
   that conv's operand gather), grouped conv, transposed conv (kernel == stride: ``deconv``), GhostConv's
   depthwise 5x5 + concat with Ghost's shortcut (``ghost``), max-pool, upsample, concat, Detect/IDetect heads,
   the Classify head (``classify``: global average pool + the centre tap of its conv, ycx_classify).
2. Passes: nearest-x2 upsample fused into its producing conv's store
   (YCX_OUT_NHWC_UP2); the SPPCSPC 5/9/13 pools run as a k5 cascade (exact for
   max with -inf padding); Contract, Expand and a Focus that reads an activation move their pixels with
   ycx_space_depth (``depth``; a Focus on the image is ReOrg + Conv: ``stem_reorg``); every concat
   input that a kernel produces is written straight into its channel slice of the concat buffer (Concat costs nothing;
   a copy kernel runs only for inputs that cannot alias).
3. Bind the schedule to memory: ``schedule.Schedule`` decides, without a device, which launches
   run the graph (stem pair, conv pair and trio, pooled 1x1, pool cascade) and which buffers
   they need. Allocate one NHWC device buffer per value (no reuse: a yolov7 bs=32 640x640 plan
   is ~10 GB of bf16 activations, small next to 288 GB HBM), move the packed weights and descriptors
   that ``ycx.pack`` decides, also without a device, onto it ([cout_pad][kh][kw][cin], bf16 or fp32)
   and emit one op per launch into the ctypes array consumed by the native loop ``ycx_run_ops`` (or
   a HIP graph).
"""
from __future__ import annotations

import ctypes
import math
import os

import numpy as np
import torch
from torch import nn

from . import _lib as L
from . import pack
from .nets.common import (SP, SPP, SPPCSPC, SPPF, MP, Bottleneck, BottleneckCSPA, BottleneckCSPB, BottleneckCSPC,
                          Classify, Concat, Contract, Conv, DownC, Expand, Focus, Ghost, GhostConv, ReOrg, RepConv, Res,
                          RobustConv, RobustConv2)
from .nets.detect import Detect, IAuxDetect, IBin, IDetect
from .pack import pack_deconv_weights, pack_fp8_weights  # noqa: F401  (re-exported)
from .schedule import Schedule, cascade_fits, cout_pad  # noqa: F401  (re-exported)


class Buf:
    __slots__ = ('n', 'h', 'w', 'c', 'tensor')

    def __init__(self, n, h, w, c):
        self.n, self.h, self.w, self.c, self.tensor = n, h, w, c, None


class Val:
    """An activation: channels [coff, coff + c) of an NHWC buffer."""
    __slots__ = ('n', 'h', 'w', 'c', 'buf', 'coff', 'producer', 'consumers', 'role')

    def __init__(self, n, h, w, c, role='act'):
        self.n, self.h, self.w, self.c = n, h, w, c
        self.buf, self.coff, self.producer, self.consumers, self.role = None, 0, None, [], role


class Node:
    __slots__ = ('kind', 'inputs', 'out', 'p')

    def __init__(self, kind, inputs, out, **p):
        self.kind, self.inputs, self.out, self.p = kind, inputs, out, p


def _pair(v):
    return v if isinstance(v, (tuple, list)) else (v, v)


def _square(v, what):
    a, b = _pair(v)
    if a != b:
        raise NotImplementedError(f"ycx: non-square {what} {v}")
    return int(a)


def fold_bn(weight, bn):
    """conv weight (+BN) -> float64 (W, b): W*gamma/std, beta - mean*gamma/std
    (nets/common.py:14-17, 503-529)."""
    w = weight.detach().to('cpu', torch.float64)
    if bn is None:
        return w, torch.zeros(w.shape[0], dtype=torch.float64)
    std = (bn.running_var.detach().to('cpu', torch.float64) + bn.eps).sqrt()
    t = bn.weight.detach().to('cpu', torch.float64) / std
    b = bn.bias.detach().to('cpu', torch.float64) - bn.running_mean.detach().to('cpu', torch.float64) * t
    return w * t.reshape(-1, 1, 1, 1), b


def fold_repconv(m: RepConv):
    """RepConv -> one 3x3 conv (get_equivalent_kernel_bias, nets/common.py:488-529)."""
    if hasattr(m, 'rbr_reparam'):
        c = m.rbr_reparam
        b = c.bias.detach().to('cpu', torch.float64) if c.bias is not None else torch.zeros(c.out_channels,
                                                                                               dtype=torch.float64)
        return c.weight.detach().to('cpu', torch.float64), b
    k3, b3 = fold_bn(m.rbr_dense[0].weight, m.rbr_dense[1])
    k1, b1 = fold_bn(m.rbr_1x1[0].weight, m.rbr_1x1[1])
    k = k3 + torch.nn.functional.pad(k1, [1, 1, 1, 1])
    b = b3 + b1
    if m.rbr_identity is not None:
        idk = torch.zeros_like(k3)
        input_dim = m.in_channels // m.groups
        for i in range(m.in_channels):
            idk[i, i % input_dim, 1, 1] = 1.0
        kid, bid = fold_bn(idk, m.rbr_identity)
        k, b = k + kid, b + bid
    return k, b


def act_of(mod):
    if isinstance(mod, nn.SiLU):
        return L.ACT_SILU, 0.0
    if isinstance(mod, nn.LeakyReLU):
        return L.ACT_LEAKY, float(mod.negative_slope)
    if isinstance(mod, nn.Identity) or mod is None:
        return L.ACT_NONE, 0.0
    raise NotImplementedError(f"ycx: activation {type(mod).__name__} has no HIP epilogue")


# what ycx_conv2d_grouped takes (include/ycx.h): channels per group (cin_g == cout_g), kernel sizes and strides;
# k 11 and strides 4, 8 for a depthwise conv (cin_g 1) only
GCONV_CIN_G = (1, 2, 4, 8, 16)
GCONV_K = (3, 5, 7, 11)
GCONV_S = (1, 2, 4, 8)
# what ycx_deconv2d takes: kernel == stride
DECONV_S = (2, 4, 8)
# what ycx_space_depth takes: the gain (Focus: 2), and the contiguous channel run a multiple of DEPTH_RUN
DEPTH_GAIN = (2, 3, 4)
DEPTH_RUN = 8
DEPTH_NAME = {L.SD_CONTRACT: 'contract', L.SD_EXPAND: 'expand', L.SD_FOCUS: 'focus'}
# what ycx_classify takes: a channel slice that is a multiple of CLASSIFY_RUN wide
CLASSIFY_RUN = 8


class Graph:
    def __init__(self):
        self.nodes = []

    def add(self, kind, inputs, out, **p):
        if kind != 'stem_reorg' and any(v.role == 'reorg' for v in inputs):
            raise NotImplementedError("ycx: ReOrg is lowered only into the Conv (k3, p1, groups 1) that reads it; "
                                      f"here a '{kind}' reads it")
        node = Node(kind, list(inputs), out, **p)
        out.producer = node
        for v in inputs:
            v.consumers.append(node)
        self.nodes.append(node)
        return out

    # ---- primitive ops ----
    def conv(self, x: Val, w64, b64, k, s, p, act=(L.ACT_NONE, 0.0), residual=None, head=False, groups=1):
        cout, cin = int(w64.shape[0]), int(w64.shape[1])
        if groups > 1:
            return self._gconv(x, w64, b64, k, s, p, act, residual, head, groups)
        if cin != x.c:
            raise NotImplementedError(f"ycx: grouped/mismatched conv (cin {cin} vs input {x.c})")
        ho, wo = (x.h + 2 * p - k) // s + 1, (x.w + 2 * p - k) // s + 1
        out = Val(x.n, ho, wo, cout, role='output' if head else 'act')
        ins = [x] + ([residual] if residual is not None else [])
        kind = 'stem' if x.role == 'input' else 'stem_reorg' if x.role == 'reorg' else 'conv'
        if kind != 'conv' and residual is not None:
            raise NotImplementedError("ycx: residual on the input conv")
        if kind == 'stem_reorg' and not (k == 3 and p == 1 and s in (1, 2) and not head):
            raise NotImplementedError("ycx: ReOrg is lowered only into a 3x3 / pad-1 Conv of stride 1 or 2 "
                                      f"(ycx_stem_conv_reorg); got k{k} s{s} p{p}")
        return self.add(kind, ins, out, w=w64, b=b64, k=k, s=s, p=p, act=act[0], slope=act[1],
                        residual=residual, ho=ho, wo=wo, layout=L.OUT_NCHW_F32 if head else L.OUT_NHWC)

    def _gconv(self, x, w64, b64, k, s, p, act, residual, head, groups):
        """A grouped conv (weights [cout][cin_g][k][k]) as a node of its own kind, 'gconv'
        (ycx_conv2d_grouped): every pass that fuses, merges, pairs or splits convs looks for
        kind 'conv' and so leaves it alone; only the concat-slice aliasing takes it."""
        cout, cin_g = int(w64.shape[0]), int(w64.shape[1])
        if x.role in ('input', 'reorg'):
            raise NotImplementedError("ycx: grouped conv on the model input")
        if cin_g * groups != x.c or cout % groups:
            raise NotImplementedError(f"ycx: grouped/mismatched conv (cin {cin_g} x {groups} groups vs input {x.c})")
        cout_g = cout // groups
        wide = k == 11 or s in (4, 8)  # the depthwise-only shapes
        if not (cin_g == cout_g and cin_g in GCONV_CIN_G and k in GCONV_K and p == k // 2 and s in GCONV_S
                and (cin_g == 1 or not wide) and cout % 8 == 0 and not head):
            raise NotImplementedError(
                f"ycx: grouped conv with cin_g {cin_g}, cout_g {cout_g}, k {k} (s {s}, p {p}, cout {cout}) has no HIP "
                f"kernel: ycx_conv2d_grouped takes cin_g == cout_g in {GCONV_CIN_G}, k in {GCONV_K}, p == k // 2, "
                f"s in {GCONV_S} (k 11 and s 4, 8: depthwise only), cout % 8 == 0")
        ho, wo = (x.h + 2 * p - k) // s + 1, (x.w + 2 * p - k) // s + 1
        ins = [x] + ([residual] if residual is not None else [])
        return self.add('gconv', ins, Val(x.n, ho, wo, cout), w=w64, b=b64, k=k, s=s, p=p, act=act[0], slope=act[1],
                        residual=residual, ho=ho, wo=wo, layout=L.OUT_NHWC, groups=groups)

    def deconv(self, x: Val, w64, b64, s, act=(L.ACT_NONE, 0.0)):
        """A transposed conv with kernel == stride == s (weights [cin][cout][s][s], torch's layout) as a
        node of its own kind, 'deconv' (ycx_deconv2d): like 'gconv', no conv-fusing pass looks at it;
        only the concat-slice aliasing takes it."""
        cin, cout = int(w64.shape[0]), int(w64.shape[1])
        if x.role in ('input', 'reorg'):
            raise NotImplementedError("ycx: transposed conv on the model input")
        if tuple(w64.shape[2:]) != (s, s) or s not in DECONV_S:
            raise NotImplementedError(f"ycx: transposed conv with kernel {tuple(w64.shape[2:])}, stride {s} has no HIP "
                                      f"kernel: ycx_deconv2d takes kernel_size == stride in {DECONV_S}")
        if cin != x.c or cin % 8 or cout % 8:
            raise NotImplementedError(f"ycx: transposed conv with cin {cin} (input {x.c}), cout {cout}: ycx_deconv2d "
                                      f"takes cin == the input's channels, cin % 8 == 0, cout % 8 == 0")
        ho, wo = x.h * s, x.w * s
        return self.add('deconv', [x], Val(x.n, ho, wo, cout), w=w64, b=b64, k=s, s=s, p=0, act=act[0], slope=act[1],
                        residual=None, ho=ho, wo=wo, layout=L.OUT_NHWC)

    def ghost(self, y: Val, w64, b64, act=(L.ACT_NONE, 0.0), residual=None):
        """GhostConv's cat[y, cv2(y)] (+ residual over all 2c channels) as a node of its own kind, 'ghost'
        (ycx_ghost_dw); w64 [c][1][5][5] is cv2's folded depthwise 5x5 / s1 / p2 weight. Like 'gconv' and
        'deconv', no conv-fusing pass looks at it; the concat-slice aliasing takes it, and a residual-free
        one gets y placed in the first half of its own output (``Plan._passes``)."""
        c = int(w64.shape[0])
        if y.role in ('input', 'reorg'):
            raise NotImplementedError("ycx: GhostConv on the model input")
        if tuple(w64.shape) != (y.c, 1, 5, 5):
            raise NotImplementedError(f"ycx: ghost conv weight {tuple(w64.shape)} on {y.c} channels: ycx_ghost_dw takes "
                                      f"a depthwise 5x5 over the hidden map")
        if c % 8:
            raise NotImplementedError(f"ycx: ghost conv on {c} hidden channels: ycx_ghost_dw takes c % 8 == 0 "
                                      f"(a GhostConv of c2 % 16 == 0)")
        if residual is not None and (residual.n, residual.h, residual.w, residual.c) != (y.n, y.h, y.w, 2 * c):
            raise ValueError(f"ycx: Ghost shortcut of shape {(residual.n, residual.h, residual.w, residual.c)} "
                             f"on an output of {(y.n, y.h, y.w, 2 * c)}")
        ins = [y] + ([residual] if residual is not None else [])
        return self.add('ghost', ins, Val(y.n, y.h, y.w, 2 * c), w=w64, b=b64, k=5, s=1, p=2, act=act[0],
                        slope=act[1], residual=residual, ho=y.h, wo=y.w, layout=L.OUT_NHWC, groups=c)

    def pool(self, x: Val, k, s, p):
        if x.role == 'input':
            raise NotImplementedError("ycx: pooling the raw input image")
        ho, wo = (x.h + 2 * p - k) // s + 1, (x.w + 2 * p - k) // s + 1
        return self.add('pool', [x], Val(x.n, ho, wo, x.c), k=k, s=s, p=p)

    def reorg(self, x: Val):
        """ReOrg (nets/common.py:43-51) of the model input: no node and no buffer, only the
        (n, h/2, w/2, 4c) view that the one Conv reading it gathers through (``stem_reorg``)."""
        if x.role != 'input':
            raise NotImplementedError("ycx: ReOrg is lowered only on the model input (layer 0 of the P6 "
                                      "configs); elsewhere it is out of scope for the HIP inference path")
        if x.h % 2 or x.w % 2:
            raise ValueError(f"ycx: ReOrg needs even image sides, got {x.h} x {x.w} (the reference's torch.cat "
                             f"fails there)")
        return Val(x.n, x.h // 2, x.w // 2, 4 * x.c, role='reorg')

    def depth(self, x: Val, mode, gain):
        """Contract / Expand (nets/common.py:787-812), or the pixel-phase concat of a Focus that reads an
        activation (:767), as a node of its own kind, 'depth' (ycx_space_depth): a pure move, so the
        concat-slice aliasing takes it and an fp8 plan ties its input and output to one scale."""
        what = DEPTH_NAME[mode].capitalize()
        if x.role in ('input', 'reorg'):
            raise NotImplementedError(f"ycx: {what} on the model input (ycx_space_depth reads an NHWC activation, "
                                      f"not the image; a Focus there is lowered into ycx_stem_conv_reorg)")
        limits = (f"ycx_space_depth takes a gain in {DEPTH_GAIN} (Focus: 2) and a contiguous channel run (c for "
                  f"Contract and Focus, c / gain^2 for Expand) that is a multiple of {DEPTH_RUN}")
        if isinstance(gain, bool) or not isinstance(gain, int) or gain not in DEPTH_GAIN or \
                (mode == L.SD_FOCUS and gain != 2):
            raise NotImplementedError(f"ycx: {what} with gain {gain!r} has no HIP kernel: {limits}")
        ss = gain * gain
        if mode == L.SD_EXPAND:
            if x.c % ss:
                raise ValueError(f"ycx: Expand({gain}) needs channels divisible by {ss}, got {x.c} (the reference's "
                                 f"view fails there)")
            out, run = Val(x.n, x.h * gain, x.w * gain, x.c // ss), x.c // ss
        else:
            if x.h % gain or x.w % gain:
                raise ValueError(f"ycx: {what}({gain}) needs spatial sides divisible by {gain}, got {x.h} x {x.w} "
                                 f"(the reference's view fails there)")
            out, run = Val(x.n, x.h // gain, x.w // gain, x.c * ss), x.c
        if run % DEPTH_RUN:
            raise NotImplementedError(f"ycx: {what}({gain}) on {x.c} channels (a run of {run}) has no HIP kernel: "
                                      f"{limits}")
        return self.add('depth', [x], out, mode=mode, gain=gain)

    def classify(self, x: Val, w64, b64, k, s, p, groups):
        """Classify (nets/common.py:815-825) as a node of its own kind, 'classify' (ycx_classify): the mean over
        H x W, then the Conv2d on the 1 x 1 map. With an odd k and p == k // 2 only the centre tap meets data
        and the output is 1 x 1 for any stride, so the node keeps w64[:, :, k//2, k//2] as a [cout][c][1][1]
        weight. Its output is the model's: fp32 [n][cout], no buffer, no copy."""
        if x.role in ('input', 'reorg'):
            raise NotImplementedError("ycx: Classify on the model input (ycx_classify reads an NHWC activation, "
                                      "not the image)")
        if groups != 1 or k % 2 == 0 or p != k // 2:
            raise NotImplementedError(f"ycx: Classify with k {k}, s {s}, p {p}, g {groups} has no HIP kernel: "
                                      f"ycx_classify takes g == 1, an odd k and p == k // 2 (any s), where only the "
                                      f"conv's centre tap meets the pooled 1 x 1 map")
        cout, cin = int(w64.shape[0]), int(w64.shape[1])
        if cin != x.c:
            raise ValueError(f"ycx: Classify built for {cin} input channels reads a layer of {x.c} (the reference's "
                             f"conv fails there)")
        if x.c % CLASSIFY_RUN:
            raise NotImplementedError(f"ycx: Classify on {x.c} channels has no HIP kernel: ycx_classify takes a "
                                      f"channel slice that is a multiple of {CLASSIFY_RUN}")
        w = w64[:, :, k // 2, k // 2].reshape(cout, cin, 1, 1).contiguous()
        return self.add('classify', [x], Val(x.n, 1, 1, cout, role='output'), w=w, b=b64, k=1, s=1, p=0, ho=1, wo=1,
                        kernel=k, stride=s)

    def upsample(self, x: Val):
        return self.add('up', [x], Val(x.n, 2 * x.h, 2 * x.w, x.c))

    def concat(self, xs):
        n, h, w = xs[0].n, xs[0].h, xs[0].w
        if any((v.n, v.h, v.w) != (n, h, w) for v in xs):
            raise ValueError("ycx: Concat inputs differ in spatial size")
        return self.add('concat', xs, Val(n, h, w, sum(v.c for v in xs)))


def conv_module(g: Graph, m: Conv, x: Val, residual=None):
    c = m.conv
    if _pair(c.dilation) != (1, 1):
        raise NotImplementedError("ycx: dilated conv")
    w, b = fold_bn(c.weight, m.bn)
    return g.conv(x, w, b, _square(c.kernel_size, 'kernel'), _square(c.stride, 'stride'),
                  _square(c.padding, 'padding'), act_of(m.act), residual=residual, groups=int(c.groups))


def ghostconv_module(g: Graph, m: GhostConv, x: Val, residual=None):
    """GhostConv (nets/common.py:142-152): cv1 as an ordinary conv / gconv node, then one 'ghost' node for
    cv2, the concat and, for the second GhostConv of a Ghost block, the shortcut."""
    c = m.cv2.conv
    k, s, p = _square(c.kernel_size, 'kernel'), _square(c.stride, 'stride'), _square(c.padding, 'padding')
    if not (k == 5 and s == 1 and p == 2 and c.groups == c.in_channels == c.out_channels
            and _pair(c.dilation) == (1, 1)):
        raise NotImplementedError(f"ycx: GhostConv.cv2 with k {k}, s {s}, p {p}, groups {c.groups} on "
                                  f"{c.in_channels} -> {c.out_channels} channels has no HIP kernel: ycx_ghost_dw "
                                  f"takes the depthwise 5x5 / s1 / p2 conv")
    if x.role in ('input', 'reorg'):  # the parser's rule (nets/yolo.py), for a module lowered on its own
        raise NotImplementedError("ycx: GhostConv on the model input")
    y = conv_module(g, m.cv1, x)
    w, b = fold_bn(c.weight, m.cv2.bn)
    return g.ghost(y, w, b, act_of(m.cv2.act), residual=residual)


def focus_module(g: Graph, m: Focus, x: Val):
    """Focus (nets/common.py:759-767): its four pixel phases come in ReOrg's order, so on the image it is
    ReOrg + Conv, the ``stem_reorg`` node; on an activation a 'depth' node in focus mode, then the conv."""
    if x.role != 'input':
        return conv_module(g, m.conv, g.depth(x, L.SD_FOCUS, 2))
    c = m.conv.conv
    k, s, p = _square(c.kernel_size, 'kernel'), _square(c.stride, 'stride'), _square(c.padding, 'padding')
    if not (k == 3 and p == 1 and s in (1, 2) and c.groups == 1 and _pair(c.dilation) == (1, 1)):
        raise NotImplementedError("ycx: Focus on the model input is lowered into ycx_stem_conv_reorg, which takes a "
                                  f"3x3 / pad-1 conv of stride 1 or 2 with groups 1; got k{k} s{s} p{p} g{c.groups}")
    return conv_module(g, m.conv, g.reorg(x))


def conv_or_ghost(g: Graph, m, x: Val):
    return ghostconv_module(g, m, x) if isinstance(m, GhostConv) else conv_module(g, m, x)


def conv_or_rep(g: Graph, m, x: Val, residual=None):
    """A block's cv2: a Conv, or in the Rep blocks a RepConv folded to its one 3x3 (``fold_repconv``), a
    grouped one as a 'gconv' node within ycx_conv2d_grouped's limits."""
    if not isinstance(m, RepConv):
        return conv_module(g, m, x, residual=residual)
    w, b = fold_repconv(m)
    return g.conv(x, w, b, 3, m.stride, 1, act_of(m.act), residual=residual, groups=int(m.groups))


def ghost_module(g: Graph, m: Ghost, x: Val):
    """Ghost (nets/common.py:233-245): conv(x) + shortcut(x). The add runs over the second GhostConv's
    concat, so it is that ghost node's residual: x itself for s = 1, the shortcut's 1x1 output for s = 2."""
    first, dw, last = m.conv[0], m.conv[1], m.conv[2]
    if isinstance(m.shortcut, nn.Identity):
        c2 = 2 * last.cv2.conv.out_channels
        if x.c != c2:
            raise ValueError(f"ycx: Ghost with stride 1 needs c1 == c2, got {x.c} -> {c2} (the reference's add "
                             f"fails there)")
        r = x
    else:
        r = lower_module(g, m.shortcut, x)
    y = ghostconv_module(g, first, x)
    if not isinstance(dw, nn.Identity):
        y = conv_module(g, dw, y)
    return ghostconv_module(g, last, y, residual=r)


def fold_robustconv(m: RobustConv):
    """RobustConv's biased 1x1 with its layer scale folded in, float64 (W, b):
    (W x + b) * gamma = (gamma W) x + gamma b (nets/common.py:123-124)."""
    c = m.conv1x1
    w = c.weight.detach().to('cpu', torch.float64)
    b = c.bias.detach().to('cpu', torch.float64)
    if m.gamma is not None:
        gm = m.gamma.detach().to('cpu', torch.float64)
        w, b = w * gm.reshape(-1, 1, 1, 1), b * gm
    return w, b


def fold_robustconv2(m: RobustConv2):
    """RobustConv2's biased transposed conv with its layer scale folded in, float64 (W [cin][cout][s][s], b):
    (W^T x + b) * gamma = (gamma W)^T x + gamma b, gamma along W's second dim (nets/common.py:138-139)."""
    c = m.conv_deconv
    w = c.weight.detach().to('cpu', torch.float64)
    b = c.bias.detach().to('cpu', torch.float64)
    if m.gamma is not None:
        gm = m.gamma.detach().to('cpu', torch.float64)
        w, b = w * gm.reshape(1, -1, 1, 1), b * gm
    return w, b


def deconv_module(g: 'Graph', c: nn.ConvTranspose2d, x, w=None, b=None):
    """An nn.ConvTranspose2d (its own weights, or the folded w, b given) as a 'deconv' node; every form
    ycx_deconv2d does not take is refused by the name of the offending field."""
    k, s = _square(c.kernel_size, 'kernel_size'), _square(c.stride, 'stride')
    for field, ok in (('kernel_size', k == s), ('padding', _pair(c.padding) == (0, 0)),
                      ('output_padding', _pair(c.output_padding) == (0, 0)), ('dilation', _pair(c.dilation) == (1, 1)),
                      ('groups', c.groups == 1), ('stride', s in DECONV_S)):
        if not ok:
            raise NotImplementedError(
                f"ycx: nn.ConvTranspose2d with {field} {getattr(c, field)} (kernel_size {k}, stride {s}) has no HIP "
                f"kernel: ycx_deconv2d takes kernel_size == stride in {DECONV_S}, padding 0, output_padding 0, "
                f"dilation 1, groups 1")
    if w is None:
        w = c.weight.detach().to('cpu', torch.float64)
        b = c.bias.detach().to('cpu', torch.float64) if c.bias is not None else torch.zeros(w.shape[1],
                                                                                            dtype=torch.float64)
    return g.deconv(x, w, b, s)


def check_plan_precision(plan, precision):
    """What a plan cannot run in a given precision, raised before anything is allocated."""
    if precision == 'fp8' and any(nd.kind == 'deconv' for nd in plan.graph.nodes):
        raise NotImplementedError("ycx: transposed conv has no fp8 path (ycx_deconv2d takes bf16, fp16 and f32); "
                                  "run this model in 'fp16', 'bf16' or 'f32'")
    if precision == 'fp8' and any(nd.kind == 'ghost' for nd in plan.graph.nodes):
        raise NotImplementedError("ycx: ghost conv has no fp8 path (ycx_ghost_dw takes bf16, fp16 and f32); "
                                  "run this model in 'fp16', 'bf16' or 'f32'")
    if precision == 'fp8' and any(nd.kind == 'gconv' for nd in plan.graph.nodes):
        raise NotImplementedError("ycx: grouped conv has no fp8 path (ycx_conv2d_grouped takes bf16, fp16 and f32); "
                                  "run this model in 'fp16', 'bf16' or 'f32'")


def pool_module(g: Graph, mp: nn.MaxPool2d, x: Val):
    if mp.ceil_mode or _pair(mp.dilation) != (1, 1):
        raise NotImplementedError("ycx: ceil_mode / dilated max-pool")
    k = _square(mp.kernel_size, 'pool kernel')
    s = _square(mp.stride if mp.stride is not None else k, 'pool stride')
    return g.pool(x, k, s, _square(mp.padding, 'pool padding'))


def pyramid(g: Graph, x: Val, pools):
    """SPP-style pools of x. s=1 'same' pools whose kernels step by 4 from 5
    (5, 9, 13) run as a cascade of k=5 pools: maxpool_{a+b-1} = maxpool_a o maxpool_b
    for stride 1 with -inf padding (exact, SPPF's own identity)."""
    ks = [(_square(m.kernel_size, 'k'), _square(m.stride, 's'), _square(m.padding, 'p')) for m in pools]
    cascade = all(s == 1 and p == k // 2 for k, s, p in ks) and [k for k, _, _ in ks] == [5 + 4 * i for i in range(len(ks))]
    outs, cur = [], x
    for (k, s, p), m in zip(ks, pools):
        if cascade:
            cur = g.pool(cur, 5, 1, 2)
            outs.append(cur)
        else:
            outs.append(pool_module(g, m, x))
    return outs


def lower_module(g: Graph, m, x):
    if isinstance(m, nn.Sequential):
        for mm in m:
            x = lower_module(g, mm, x)
        return x
    if isinstance(m, Conv):
        return conv_module(g, m, x)
    if isinstance(m, RepConv):
        w, b = fold_repconv(m)
        return g.conv(x, w, b, 3, m.stride, 1, act_of(m.act), groups=int(m.groups))
    if isinstance(m, nn.Conv2d):
        w = m.weight.detach().to('cpu', torch.float64)
        b = m.bias.detach().to('cpu', torch.float64) if m.bias is not None else torch.zeros(w.shape[0],
                                                                                            dtype=torch.float64)
        if _pair(m.dilation) != (1, 1):
            raise NotImplementedError("ycx: dilated conv")
        return g.conv(x, w, b, _square(m.kernel_size, 'k'), _square(m.stride, 's'), _square(m.padding, 'p'),
                      groups=int(m.groups))
    if isinstance(m, (MP, SP)):
        return pool_module(g, m.m, x)
    if isinstance(m, ReOrg):
        return g.reorg(x)
    if isinstance(m, Focus):
        return focus_module(g, m, x)
    if isinstance(m, Contract):
        return g.depth(x, L.SD_CONTRACT, m.gain)
    if isinstance(m, Expand):
        return g.depth(x, L.SD_EXPAND, m.gain)
    if isinstance(m, DownC):  # nets/common.py:181-182
        y1 = conv_module(g, m.cv2, conv_module(g, m.cv1, x))
        return g.concat([y1, conv_module(g, m.cv3, pool_module(g, m.mp, x))])
    if isinstance(m, nn.MaxPool2d):
        return pool_module(g, m, x)
    if isinstance(m, Concat):
        if m.d != 1:
            raise NotImplementedError("ycx: Concat along a non-channel dim")
        return g.concat(x)
    if isinstance(m, nn.Upsample):
        sf = m.scale_factor
        sf = sf[0] if isinstance(sf, (tuple, list)) else sf
        if m.mode != 'nearest' or m.size is not None or float(sf) != 2.0:
            raise NotImplementedError("ycx: only nn.Upsample(None, 2, 'nearest') is supported")
        return g.upsample(x)
    if isinstance(m, nn.Identity):
        return x
    if isinstance(m, Bottleneck):  # RepBottleneck too: its cv2 is a RepConv (nets/common.py:617-622)
        y = conv_module(g, m.cv1, x)
        return conv_or_rep(g, m.cv2, y, residual=x if m.add else None)
    # ResX too (nets/common.py:212-230), and RepRes / RepResX, whose cv2 is a RepConv (:649-686); the shortcut is
    # cv3's epilogue residual
    if isinstance(m, Res):
        y = conv_or_rep(g, m.cv2, conv_module(g, m.cv1, x))
        return conv_module(g, m.cv3, y, residual=x if m.add else None)
    if isinstance(m, RobustConv):  # nets/common.py:121-124; its channels_last call changes no value
        w, b = fold_robustconv(m)
        return g.conv(conv_module(g, m.conv_dw, x), w, b, 1, 1, 0)
    if isinstance(m, RobustConv2):  # nets/common.py:137-139
        w, b = fold_robustconv2(m)
        return deconv_module(g, m.conv_deconv, conv_module(g, m.conv_strided, x), w, b)
    if isinstance(m, nn.ConvTranspose2d):
        return deconv_module(g, m, x)
    if isinstance(m, GhostConv):
        return ghostconv_module(g, m, x)
    if isinstance(m, Ghost):
        return ghost_module(g, m, x)
    if isinstance(m, Classify):
        c = m.conv
        if not isinstance(x, Val):
            raise NotImplementedError("ycx: Classify reads one layer, got a list")
        if _pair(c.dilation) != (1, 1):
            raise NotImplementedError("ycx: dilated conv")
        w = c.weight.detach().to('cpu', torch.float64)
        b = c.bias.detach().to('cpu', torch.float64) if c.bias is not None else torch.zeros(w.shape[0],
                                                                                            dtype=torch.float64)
        return g.classify(x, w, b, _square(c.kernel_size, 'kernel'), _square(c.stride, 'stride'),
                          _square(c.padding, 'padding'), int(c.groups))
    if isinstance(m, SPPCSPC):  # GhostSPPCSPC too: its cv1 .. cv7 are GhostConvs (nets/common.py:269-280)
        cv = conv_or_ghost
        x1 = cv(g, m.cv4, cv(g, m.cv3, cv(g, m.cv1, x)))
        y1 = cv(g, m.cv6, cv(g, m.cv5, g.concat([x1] + pyramid(g, x1, list(m.m)))))
        y2 = cv(g, m.cv2, x)
        return cv(g, m.cv7, g.concat([y1, y2]))
    if isinstance(m, SPPF):
        x1 = conv_module(g, m.cv1, x)
        y1 = pool_module(g, m.m, x1)
        y2 = pool_module(g, m.m, y1)
        y3 = pool_module(g, m.m, y2)
        return conv_module(g, m.cv2, g.concat([x1, y1, y2, y3]))
    if isinstance(m, SPP):
        x1 = conv_module(g, m.cv1, x)
        return conv_module(g, m.cv2, g.concat([x1] + pyramid(g, x1, list(m.m))))
    # the CSP blocks: also their Res*CSP* / ResX*CSP* / GhostCSP* subclasses, whose m is a Sequential of Res / Ghost
    if isinstance(m, BottleneckCSPA):
        y1 = lower_module(g, m.m, conv_module(g, m.cv1, x))
        return conv_module(g, m.cv3, g.concat([y1, conv_module(g, m.cv2, x)]))
    if isinstance(m, BottleneckCSPB):
        x1 = conv_module(g, m.cv1, x)
        return conv_module(g, m.cv3, g.concat([lower_module(g, m.m, x1), conv_module(g, m.cv2, x1)]))
    if isinstance(m, BottleneckCSPC):
        y1 = conv_module(g, m.cv3, lower_module(g, m.m, conv_module(g, m.cv1, x)))
        return conv_module(g, m.cv4, g.concat([y1, conv_module(g, m.cv2, x)]))
    if isinstance(m, Detect):
        outs = []
        for conv, idx in m.heads_in_output_order():
            w = conv.weight.detach().to('cpu', torch.float64)
            b = conv.bias.detach().to('cpu', torch.float64)
            outs.append(g.conv(x[idx], w, b, 1, 1, 0, head=True))
        return outs
    # IAuxDetect too: its eval uses the main heads only (x[:nl]); IBin: the same convs at its own width
    # (nets/ibin.py:46-47), the binned w/h decode reads their fp32 logits (ycx_ibin_decode)
    if isinstance(m, (IDetect, IBin)):
        outs = []
        for i in range(m.nl):
            conv = m.m[i]
            # x_i = im * (conv(x_i + ia)) = (im*W) x + im*(b + W.ia)   (nets/idetect.py:30-31)
            w = conv.weight.detach().to('cpu', torch.float64)
            b = conv.bias.detach().to('cpu', torch.float64)
            ia = m.ia[i].implicit.detach().to('cpu', torch.float64).reshape(-1)
            im = m.im[i].implicit.detach().to('cpu', torch.float64).reshape(-1)
            b = (b + w[:, :, 0, 0] @ ia) * im
            w = w * im.reshape(-1, 1, 1, 1)
            outs.append(g.conv(x[i], w, b, 1, 1, 0, head=True))
        return outs
    raise NotImplementedError(f"ycx: no HIP lowering for {type(m).__name__}")


# Development A/B of tile choices: YCX_TILE_MAP="16:24/26,18:26" replaces the picked
# tile 16 by 24 where cout_pad allows, else 26; "16<600:25/26" only where the picked tile
# launches fewer than 600 workgroups (never set in the product path).
_TILE_MAP = {}
_TILE_SHAPE = {15: (64, 256), 16: (128, 128), 18: (64, 128), 24: (256, 256), 25: (256, 128), 26: (128, 256)}
for _kv in os.environ.get('YCX_TILE_MAP', '').split(','):
    if _kv:
        _a, _b = _kv.split(':')
        _t, _, _cap = _a.partition('<')
        _TILE_MAP[int(_t)] = (int(_cap) if _cap else 1 << 62, [int(t) for t in _b.split('/')])
# A/B switch: YCX_NO_KSPLIT=1 runs every conv unsplit even where ycx_conv_pick_ksplit splits its K loop
_NO_KSPLIT = bool(os.environ.get('YCX_NO_KSPLIT'))
# A/B switch: YCX_NO_SILU_PS=1 packs SiLU convs unscaled and runs the plain YCX_ACT_SILU epilogue
_NO_SILU_PS = bool(os.environ.get('YCX_NO_SILU_PS'))


class Plan:
    """Device-independent lowering of a Model for one input shape: the graph
    after all passes, its outputs and its algorithmic FLOPs."""

    def __init__(self, model, shape):
        if len(shape) != 4:
            raise ValueError(f"ycx: expected an NCHW input, got shape {shape}")
        self.shape = tuple(int(s) for s in shape)
        n, c, h, w = self.shape
        g = Graph()
        self.input_val = Val(n, h, w, c, role='input')
        ys, x = [], self.input_val
        for m in model.model:  # nets/yolo.py:145-151
            if m.f != -1:
                x = ys[m.f] if isinstance(m.f, int) else [x if j == -1 else ys[j] for j in m.f]
            x = lower_module(g, m, x)
            ys.append(x)
        for v in ys:  # a ReOrg view feeds exactly one node, its stem_reorg conv (Graph.add refuses other kinds)
            if isinstance(v, Val) and v.role == 'reorg' and (len(v.consumers) != 1 or x is v):
                raise NotImplementedError("ycx: ReOrg is lowered only with one Conv (k3, p1, groups 1) as its "
                                          f"only consumer; it has {len(v.consumers)} consumers")
        self.is_list = isinstance(x, list)
        self.out_vals = list(x) if self.is_list else [x]
        for nd in g.nodes:  # a Classify's [n][c2] logits are the model's output, nothing reads them
            if nd.kind == 'classify' and (nd.out is not x or nd.out.consumers):
                raise NotImplementedError("ycx: Classify is lowered only as the model's last layer")
        self.graph = g
        self._eliminate_dead()
        self._passes()

    @property
    def conv_flops(self):
        """Algorithmic FLOPs of the folded convs of every kind and of a Classify head's dense layer (``pack.flops``)."""
        return sum(pack.flops(nd) for nd in self.graph.nodes if nd.kind in pack.PACKED_KINDS)

    def counts(self):
        """Node kinds after the passes; 'conv' counts the original convs (a merged
        sibling pair counts 2), 'merged' the merged nodes."""
        c = {}
        for nd in self.graph.nodes:
            kind = nd.kind
            if kind == 'conv' and nd.p.get('parts', 1) > 1:
                c['merged'] = c.get('merged', 0) + 1
                c['conv'] = c.get('conv', 0) + nd.p['parts'] - 1
            if kind == 'concat':
                c['copy'] = c.get('copy', 0) + len(nd.p['copies'])
            c[kind] = c.get(kind, 0) + 1
        return c

    def _eliminate_dead(self):
        """Drop nodes whose value nobody reads (IAuxDetect's aux branch in eval:
        nets/iaux_detect.py:32-33 computes it, :49 discards it)."""
        g = self.graph
        live = {id(v) for v in self.out_vals}
        keep = []
        for node in reversed(g.nodes):
            if id(node.out) in live:
                keep.append(node)
                live.update(id(v) for v in node.inputs)
            else:
                for v in node.inputs:
                    v.consumers = [c for c in v.consumers if c is not node]
        g.nodes = keep[::-1]

    def _passes(self):
        g = self.graph
        for v in self.out_vals:
            if v.role != 'output':  # not a head conv: convert NHWC -> fp32 NCHW at the end
                o = Val(v.n, v.h, v.w, v.c, role='output')
                g.add('tonchw', [v], o)
                self.out_vals[self.out_vals.index(v)] = o
        # Fuse nearest-x2 upsample into the producing conv's store.
        keep = []
        for node in g.nodes:
            if node.kind == 'up':
                v = node.inputs[0]
                prod = v.producer
                if prod is not None and prod.kind == 'conv' and len(v.consumers) == 1 and v.role == 'act':
                    prod.out = node.out
                    prod.p['layout'] = L.OUT_NHWC_UP2
                    node.out.producer = prod
                    continue
            keep.append(node)
        g.nodes = keep
        # Concat: producers write their channel slice directly when they can.
        for node in g.nodes:
            if node.kind != 'concat':
                continue
            out = node.out
            out.buf = Buf(out.n, out.h, out.w, out.c)
            copies, off = [], 0
            for v in node.inputs:
                if v.buf is None and v.role == 'act' and v.producer is not None and \
                        v.producer.kind in ('conv', 'stem', 'stem_reorg', 'gconv', 'deconv', 'ghost', 'pool', 'up',
                                            'depth'):
                    v.buf, v.coff = out.buf, off
                else:
                    copies.append((v, off))
                off += v.c
            node.p['copies'] = copies
        # A residual-free ghost node runs in place: its hidden map y, when only it reads y, is stored by
        # y's producer straight into the first half of the ghost's output, so no byte is copied. With a
        # residual the first half is y + r, and y keeps a buffer of its own.
        for node in g.nodes:
            y, out = node.inputs[0] if node.kind == 'ghost' else None, node.out
            if y is None or node.p['residual'] is not None or out.role != 'act':
                continue
            if y.buf is None and y.role == 'act' and len(y.consumers) == 1 and y.producer is not None and \
                    y.producer.kind in ('conv', 'gconv') and y.producer.p['layout'] == L.OUT_NHWC:
                if out.buf is None:
                    out.buf = Buf(out.n, out.h, out.w, out.c)
                y.buf, y.coff = out.buf, out.coff
        for node in g.nodes:
            v = node.out
            if v.buf is None and v.role == 'act':
                v.buf = Buf(v.n, v.h, v.w, v.c)
        if not os.environ.get("YCX_NO_SIBLING_MERGE"):  # A/B switch for the bench
            self._merge_sibling_1x1()

    def _merge_sibling_1x1(self):
        """Two 1x1 convs that read the same activation and write adjacent channel
        slices of one buffer (ELAN's cv1/cv2 pair feeding its concat, e.g.
        cfg/net/yolov7.yaml:17-18) become one conv with the weights stacked: the
        input is read once and the GEMM is twice as wide. Every output channel
        is the same dot product over the same K as before."""
        g = self.graph

        def mergeable(nd):
            p = nd.p
            return (nd.kind == 'conv' and p['k'] == 1 and p['s'] == 1 and p['p'] == 0 and p['residual'] is None
                    and p['layout'] == L.OUT_NHWC and nd.out.role == 'act' and nd.out.buf is not None)

        changed = True
        while changed:
            changed = False
            cands = [nd for nd in g.nodes if mergeable(nd)]
            for a in cands:
                for b in cands:
                    if a is b or a.inputs[0] is not b.inputs[0]:
                        continue
                    if (a.p['act'], a.p['slope']) != (b.p['act'], b.p['slope']):
                        continue
                    va, vb = a.out, b.out
                    if va.buf is not vb.buf or va.coff + va.c != vb.coff:
                        continue
                    out = Val(va.n, va.h, va.w, va.c + vb.c)
                    out.buf, out.coff = va.buf, va.coff
                    w = torch.cat([a.p['w'], b.p['w']], 0)
                    bias = torch.cat([a.p['b'], b.p['b']], 0)
                    m = Node('conv', [a.inputs[0]], out, **dict(a.p, w=w, b=bias,
                                                               parts=a.p.get('parts', 1) + b.p.get('parts', 1)))
                    out.producer = m
                    va.producer = vb.producer = m  # the halves stay valid views for their consumers
                    x = a.inputs[0]
                    x.consumers = [c for c in x.consumers if c is not a and c is not b] + [m]
                    i = min(g.nodes.index(a), g.nodes.index(b))
                    g.nodes = [nd for nd in g.nodes if nd is not a and nd is not b]
                    g.nodes.insert(i, m)
                    changed = True
                    break
                if changed:
                    break


class Engine:
    """A compiled plan bound to device memory for one (input shape, device, precision)."""

    def __init__(self, model, shape, device, precision='bf16', fuse_stem2=True, fp8_amax=None, prepacked=None,
                 fuse_pool=True, fuse_pair=True, fuse_pair_pool=True):
        if device.type != 'cuda':
            raise RuntimeError("ycx: the HIP path needs the model input on a ROCm device (tensor.to('cuda')); "
                               "there is no CPU path")
        self.plan = Plan(model, shape)
        check_plan_precision(self.plan, precision)
        self.shape, self.device, self.precision = self.plan.shape, device, precision
        self.dtype = {'bf16': torch.bfloat16, 'f32': torch.float32, 'fp8': torch.float8_e4m3fn,
                      'fp16': torch.float16}[precision]
        self.dt = {'bf16': L.DT_BF16, 'f32': L.DT_F32, 'fp8': L.DT_FP8, 'fp16': L.DT_F16}[precision]
        self.schedule = Schedule(self.plan, precision, fuse_stem2, fuse_pool, fuse_pair, fuse_pair_pool)
        self.prepacked = prepacked  # {'p<i>': packed tensor} from ycx.prepack (skips folding / packing)
        self.graph_exec = None
        self.graph, self.out_vals, self.is_list = self.plan.graph, self.plan.out_vals, self.plan.is_list
        self.scales = {}
        if self.dt == L.DT_FP8:
            if fp8_amax is None:
                raise ValueError("ycx: an fp8 engine needs calibration amax values (Model.calibrate_fp8)")
            self._assign_fp8_scales(fp8_amax)
        self._build()

    def activation_bufs(self):
        """The plan's activation buffers in allocation order (the order of
        ``self.buffers``; fp8 calibration keys its amax list on it)."""
        return self.schedule.activation_bufs

    def _assign_fp8_scales(self, amax):
        """One power-of-two scale per group of buffers tied by a pool or a copy
        (max-pool, nearest upsample, concat copies and space/depth moves leave bytes unchanged):
        s = 2^floor(log2(224 / amax)), i.e. the calibrated max lands in
        [224, 448) with 2x headroom below the e4m3 limit. Power-of-two scales
        make every rescale exact."""
        bufs = self.activation_bufs()
        if len(amax) != len(bufs) or any(a.get('c') != b.c for a, b in zip(amax, bufs)):
            raise ValueError("ycx: fp8 calibration was recorded on a different plan")
        parent = {id(b): id(b) for b in bufs}

        def find(i):
            while parent[i] != i:
                parent[i] = parent[parent[i]]
                i = parent[i]
            return i
        for nd in self.graph.nodes:
            if nd.kind in ('pool', 'up', 'concat', 'depth'):
                ins = [v for v in nd.inputs if v.buf is not None]
                if nd.out.buf is None:
                    continue
                for v in ins:
                    parent[find(id(v.buf))] = find(id(nd.out.buf))
        gmax = {}
        for a, b in zip(amax, bufs):
            r = find(id(b))
            gmax[r] = max(gmax.get(r, 0.0), float(a['amax']))
        for b in bufs:
            m = gmax[find(id(b))]
            self.scales[id(b)] = 2.0 ** math.floor(math.log2(224.0 / m)) if m > 0 and math.isfinite(m) else 1.0

    def _scale(self, v):
        return pack.scale_of(self.scales, v)

    def _conv_bytes(self, d, wt, **kw):
        return pack.conv_bytes(d, wt, self.dtype.itemsize, **kw)

    def _pair_op(self, a, b, c=None, pool=None, store_a=False):
        """One OP_CONV_PAIR for the chain a -> b (``schedule.conv_pairs``); with c (``schedule.pair_pools``)
        also the 1x1 conv on the max-pool of a's output. store_a: a's map is written."""
        da, wa, ba, fa, shape = self._conv_parts(a)
        db, wb, bb, fb, _ = self._conv_parts(b)
        op = L.Op()
        op.kind = L.OP_CONV_PAIR
        op.d.pair[0], op.d.pair[1] = da, db
        idx = len(self.op_info)
        op.in_ = self._val_ptr(a.inputs[0], idx, 'in_')
        op.weight, op.bias = wa.data_ptr(), ba.data_ptr()
        op.weight2, op.bias2 = wb.data_ptr(), bb.data_ptr()
        op.out = self._val_ptr(a.out, idx, 'out') if store_a else None
        op.out2 = self._val_ptr(b.out, idx, 'out2')
        isz = self.dtype.itemsize
        nbytes = (self._conv_bytes(da, wa, out_bytes=store_a) +
                  self._conv_bytes(db, wb) - db.n * db.h * db.w * db.cin * isz)  # y1 stays on chip
        info = dict(kind='conv_pair', name='wres1x1_pair', flops=fa + fb, shape=shape, parts=2,
                    shape2=(db.n, db.h, db.w, db.cin, db.cout, 1, 1))
        if c is not None:
            dc, wc, bc, fc, _ = self._conv_parts(c, pool=pool)
            op.conv3 = dc
            op.weight3, op.bias3 = wc.data_ptr(), bc.data_ptr()
            op.out3 = self._val_ptr(c.out, idx, 'out3')
            nbytes += self._conv_bytes(dc, wc, pooled=True) - 4 * dc.n * dc.h * dc.w * dc.cin * isz  # nor is it read back
            info.update(name='wres1x1_pair+mp_conv', flops=fa + fb + fc, parts=3,
                        shape3=(dc.n, dc.h, dc.w, dc.cin, dc.cout, 1, 1))
        self.op_info.append(dict(info, bytes=nbytes))
        return op

    def _build(self):
        dev, dt = self.device, self.dtype
        self.buffers, self.params = [], []
        self.packed = {}  # {'p<i>': packed tensor}, named by graph position (``pack.conv_index``)
        self._conv_index = pack.conv_index(self.graph.nodes)
        for b in self.schedule.activation_bufs:
            b.tensor = torch.empty((b.n, b.h, b.w, b.c), dtype=dt, device=dev)
            self.buffers.append(b.tensor)
        self.input_slots, self.output_slots, self.op_info = [], {}, []
        self._ksplit_ops = []  # (op index, workspace bytes) of the split-K convs
        self.scratch = []  # per-op workspaces of their own (a classify node's pooled means)
        self.conv_flops = 0
        emit = {'stem2': lambda la: self._stem2_op(*la.nodes),
                'conv_pair': lambda la: self._pair_op(*la.nodes, store_a=la.store_a),
                'conv': lambda la: self._conv_op(*la.nodes),
                'gconv': lambda la: self._plain_op(la.nodes[0], L.OP_GCONV, 'gconv_g{g}_k{k}s{s}'),
                'deconv': lambda la: self._plain_op(la.nodes[0], L.OP_DECONV, 'deconv_s{s}'),
                'ghost': lambda la: self._plain_op(la.nodes[0], L.OP_GHOST, 'ghost_dw'),
                'depth': lambda la: self._depth_op(la.nodes[0]),
                'classify': lambda la: self._classify_op(la.nodes[0]),
                'pool': lambda la: self._pool_op(la.nodes[0], levels=la.levels),
                'copy': lambda la: self._copy_op(la.src, la.dst, la.off, la.scale, nchw=la.nchw)}
        ops = [emit[la.kind](la) for la in self.schedule.launches]
        self.n_ops = len(ops)
        self.ops = (L.Op * max(1, self.n_ops))(*ops)
        # one fp32 workspace for every split-K conv of the plan (they run in turn on its stream)
        nws = max([b for _, b in self._ksplit_ops], default=0)
        self.workspace = torch.empty(max(1, nws // 4), dtype=torch.float32, device=dev) if nws else None
        for i, _ in self._ksplit_ops:
            self.ops[i].workspace = self.workspace.data_ptr()
        self.head_params = []
        self.head_unstored = set()  # fused head ops that do not store raw logits (enable_head_decode)
        self.fixed_outputs = None
        self.static_input = None
        self._static_bound = False

    def _val_ptr(self, v, op_index, field):
        if v.role in ('input', 'reorg'):  # a ReOrg view is read straight from the image
            self.input_slots.append((op_index, field))
            return None
        if v.role == 'output':
            self.output_slots.setdefault(id(v), []).append((op_index, field))
            return None
        return v.buf.tensor.data_ptr()

    def _packed(self, node, bf16_weights=False, silu_ps=False):
        """The node's packed weights and bias on the device (prepacked or ``pack.pack``), kept alive in
        self.params and named in self.packed by graph position."""
        i = 2 * self._conv_index[id(node)]
        if self.prepacked is not None:
            wt, bt = pack.take_prepacked(self.prepacked, i, pack.spec(node, self.precision, bf16_weights))
        else:
            wt, bt = pack.pack(node, self.precision, bf16_weights=bf16_weights, silu_ps=silu_ps,
                               in_scale=self._scale(node.inputs[0]))
        wt, bt = wt.to(self.device), bt.to(self.device)
        self.params += [wt, bt]
        self.packed[f"p{i}"], self.packed[f"p{i + 1}"] = wt, bt
        return wt, bt

    def _conv_parts(self, node, bf16_weights=False, pool=None):
        """Packed weights/bias (prepacked or ``pack.pack``; on the device, kept alive in self.params and named
        in self.packed), the descriptor (``pack.desc``), the FLOPs and the op_info shape of a conv-kind node.
        bf16_weights: 16-bit packing whatever the plan dtype (the fp8 stem2 pair computes in bf16;
        an fp16 plan's pair in fp16).
        pool: the k2 s2 pool node feeding this 1x1 conv, fused into it (``schedule.pool_convs``)."""
        # SiLU epilogues of the 16-bit / fp8 plans run pre-scaled (YCX_ACT_SILU_PS, ``pack``): dense convs only;
        # the fp32 parity plan keeps torch's silu(c) = c / (1 + e^-c)
        silu_ps = (node.kind in pack.DENSE and node.p['act'] == L.ACT_SILU and self.dt != L.DT_F32
                   and not _NO_SILU_PS)
        wt, bt = self._packed(node, bf16_weights, silu_ps)
        d = pack.desc(node, self.precision, bf16_weights=bf16_weights, silu_ps=silu_ps, scales=self.scales, pool=pool)
        flops = pack.flops(node)
        self.conv_flops += flops
        return d, wt, bt, flops, (d.n, d.h, d.w, d.cin, d.cout, d.kh, d.stride)

    def _conv_op(self, node, pool=None):
        x, out, r = node.inputs[0], node.out, node.p['residual']
        stem = node.kind in ('stem', 'stem_reorg')
        d, wt, bt, flops, shape = self._conv_parts(node, pool=pool)
        op = L.Op()
        op.kind = L.OP_STEM_REORG if node.kind == 'stem_reorg' else L.OP_STEM if stem else L.OP_CONV
        op.d.conv = d
        idx = len(self.op_info)
        op.in_ = self._val_ptr(x if pool is None else pool.inputs[0], idx, 'in_')
        op.weight, op.bias = wt.data_ptr(), bt.data_ptr()
        op.out = self._val_ptr(out, idx, 'out')
        op.residual = r.buf.tensor.data_ptr() if r is not None else None
        tile = 0 if stem else int(L.lib.ycx_conv_pick_tile(ctypes.byref(d)))
        if not stem and tile in _TILE_MAP:  # development A/B only (YCX_TILE_MAP)
            cap, alts = _TILE_MAP[tile]
            bm, bn = _TILE_SHAPE.get(tile, (0, 0))
            if not bm or -(-d.cout_pad // bm) * -(-(d.n * d.ho * d.wo) // bn) < cap:
                for t in alts:
                    if (t not in (24, 25) or d.cout_pad % 256 == 0) and (pool is None or t in (16, 18)):
                        tile = d.tile = t
                        break
        name = node.kind if stem else L.lib.ycx_conv_tile_name(tile).decode()
        if tile == 16 and d.stride == 2 and d.kh == 3 and d.kw == 3 and d.cin == 128 and pool is None:
            name += '+kcm'  # its own template instance (launch_glds: chunk-major K order), a row of its own in rocprof
        if not stem and pool is None and not _NO_KSPLIT:
            ks = int(L.lib.ycx_conv_pick_ksplit(ctypes.byref(d)))
            if ks > 1:  # split-K (r06): fp32 partials in the plan's workspace, then the ordered reduce launch
                d.k_split = ks
                self._ksplit_ops.append((len(self.op_info), int(L.lib.ycx_conv_workspace_size(ctypes.byref(d)))))
                name += f'+splitk{ks}'
        if pool is not None:
            name += '+maxpool_k2s2'
        op.d.conv = d  # ctypes copies a struct on assignment: store the final descriptor (tile map, k_split)
        kw = dict(stem=stem, pooled=pool is not None, residual=r is not None)
        nbytes = self._conv_bytes(d, wt, **kw)
        self.op_info.append(dict(kind=node.kind, name=name, flops=flops, shape=shape, parts=node.p.get('parts', 1),
                                 bytes=nbytes, out_bytes=nbytes - self._conv_bytes(d, wt, out_bytes=False, **kw)))
        return op

    def _plain_op(self, node, kind, name):
        """One OP_GCONV / OP_DECONV / OP_GHOST (ycx_conv2d_grouped, ycx_deconv2d, ycx_ghost_dw): no tile, no
        split-K, plain YCX_ACT_* epilogues. When the plan placed a ghost's y in the first half of its output,
        the input and output pointers and slices coincide and the op runs in place."""
        x, out, r = node.inputs[0], node.out, node.p['residual']
        d, wt, bt, flops, shape = self._conv_parts(node)
        op = L.Op()
        op.kind = kind
        op.d.conv = d
        op.in_ = x.buf.tensor.data_ptr()
        op.weight, op.bias = wt.data_ptr(), bt.data_ptr()
        op.out = out.buf.tensor.data_ptr()
        op.residual = r.buf.tensor.data_ptr() if r is not None else None
        inplace = kind == L.OP_GHOST and x.buf is out.buf and x.coff == out.coff
        # in place: only the second half is stored
        nbytes = self._conv_bytes(d, wt, residual=r is not None) - (
            d.n * d.h * d.w * d.cin * self.dtype.itemsize if inplace else 0)
        info = dict(kind=node.kind, name=name.format(g=d.cin // max(1, d.groups), k=d.kh, s=d.stride), flops=flops,
                    shape=shape, parts=1, bytes=nbytes,
                    out_bytes=nbytes - self._conv_bytes(d, wt, residual=r is not None, out_bytes=False))
        if kind == L.OP_GHOST:
            info.update(name=name + ('_inplace' if inplace else '') + ('+res' if r is not None else ''), inplace=inplace)
        self.op_info.append(info)
        return op

    def _stem2_op(self, stem, conv):
        ds, ws, bs, fs, _ = self._conv_parts(stem)
        dc, wc, bc, fc, shape = self._conv_parts(conv, bf16_weights=True)
        op = L.Op()
        op.kind = L.OP_STEM2
        op.d.pair[0], op.d.pair[1] = ds, dc
        idx = len(self.op_info)
        op.in_ = self._val_ptr(stem.inputs[0], idx, 'in_')
        op.weight, op.bias = ws.data_ptr(), bs.data_ptr()
        op.weight2, op.bias2 = wc.data_ptr(), bc.data_ptr()
        op.out = self._val_ptr(conv.out, idx, 'out')
        # the stem map stays in LDS: fp32 image in, both weight sets, the second conv's output out
        nbytes = (ds.n * ds.h * ds.w * ds.cin * 4 + ws.numel() * ws.element_size() + wc.numel() * wc.element_size() +
                  dc.n * dc.ho * dc.wo * dc.cout * self.dtype.itemsize)
        self.op_info.append(dict(kind='stem2', name='stem2_fused', flops=fs + fc, shape=shape, parts=2, bytes=nbytes))
        return op

    def _pool_op(self, node, levels=1):
        x, out, p = node.inputs[0], node.out, node.p
        d = L.PoolDesc()
        d.n, d.h, d.w, d.c, d.in_c_off, d.in_c_stride = x.n, x.h, x.w, x.c, x.coff, x.buf.c
        d.ho, d.wo, d.out_c_off, d.out_c_stride = out.h, out.w, out.coff, out.buf.c
        d.k, d.stride, d.pad, d.dtype, d.levels = p['k'], p['s'], p['p'], self.dt, levels
        op = L.Op()
        op.kind = L.OP_POOL
        op.d.pool = d
        op.in_, op.out = x.buf.tensor.data_ptr(), out.buf.tensor.data_ptr()
        name = f"maxpool_k{p['k']}s{p['s']}" + (f"_cascade{levels}" if levels > 1 else "")
        self.op_info.append(dict(kind='pool', name=name, flops=0,
                                 bytes=(x.n * (x.h * x.w + levels * out.h * out.w) * x.c * self.dtype.itemsize)))
        return op

    def _depth_op(self, node):
        """One OP_DEPTH (ycx_space_depth): the node's input slice moved into its output slice."""
        x, out, p = node.inputs[0], node.out, node.p
        d = L.DepthDesc()
        d.n, d.h, d.w, d.c, d.in_c_off, d.in_c_stride = x.n, x.h, x.w, x.c, x.coff, x.buf.c
        d.ho, d.wo, d.out_c_off, d.out_c_stride = out.h, out.w, out.coff, out.buf.c
        d.gain, d.mode, d.dtype = p['gain'], p['mode'], self.dt
        if any(v % DEPTH_RUN for v in (d.in_c_off, d.in_c_stride, d.out_c_off, d.out_c_stride)):
            raise NotImplementedError(f"ycx: {DEPTH_NAME[p['mode']]} between channel slices at {d.in_c_off} of "
                                      f"{d.in_c_stride} and {d.out_c_off} of {d.out_c_stride}: ycx_space_depth takes "
                                      f"offsets and strides that are multiples of {DEPTH_RUN}")
        op = L.Op()
        op.kind = L.OP_DEPTH
        op.d.depth = d
        op.in_, op.out = x.buf.tensor.data_ptr(), out.buf.tensor.data_ptr()
        self.op_info.append(dict(kind='depth', name=f"{DEPTH_NAME[p['mode']]}{p['gain']}", flops=0,
                                 bytes=2 * x.n * x.h * x.w * x.c * self.dtype.itemsize))
        return op

    def _classify_op(self, node):
        """One OP_CLASSIFY (ycx_classify): the input slice's means into a workspace of the op's own, then the
        centre-tap weights (fp32 in every precision) on them; the fp32 [n][cout] output is the model's. An fp8
        plan reads e4m3 with the producer's scale and stores fp32, so the node has no scale of its own."""
        x, out = node.inputs[0], node.out
        wt, bt = self._packed(node)
        d = L.ClassifyDesc()
        d.n, d.h, d.w, d.c, d.in_c_off, d.in_c_stride = x.n, x.h, x.w, x.c, x.coff, x.buf.c
        d.cout, d.dtype = out.c, self.dt
        d.dequant = 1.0 / self._scale(x) if self.dt == L.DT_FP8 else 1.0
        if d.in_c_off % CLASSIFY_RUN or d.in_c_stride % CLASSIFY_RUN:
            raise NotImplementedError(f"ycx: Classify on the channel slice at {d.in_c_off} of {d.in_c_stride}: "
                                      f"ycx_classify takes offsets and strides that are multiples of {CLASSIFY_RUN}")
        ws = torch.empty((x.n, x.c), dtype=torch.float32, device=self.device)
        self.scratch.append(ws)
        op = L.Op()
        op.kind = L.OP_CLASSIFY
        op.d.classify = d
        idx = len(self.op_info)
        op.in_ = x.buf.tensor.data_ptr()
        op.weight, op.bias, op.workspace = wt.data_ptr(), bt.data_ptr(), ws.data_ptr()
        op.out = self._val_ptr(out, idx, 'out')
        flops = pack.flops(node)
        self.conv_flops += flops
        nbytes = x.n * x.h * x.w * x.c * self.dtype.itemsize + 4 * (wt.numel() + bt.numel() + x.n * out.c)
        self.op_info.append(dict(kind='classify', name='classify', flops=flops, bytes=nbytes,
                                 shape=(x.n, x.h, x.w, x.c, out.c, 1, 1)))
        return op

    def _copy_op(self, x, out, off, scale, nchw=False):
        d = L.CopyDesc()
        d.n, d.h, d.w, d.c, d.in_c_off, d.in_c_stride = x.n, x.h, x.w, x.c, x.coff, x.buf.c
        d.scale, d.dtype = scale, self.dt
        op = L.Op()
        op.kind = L.OP_COPY
        idx = len(self.op_info)
        op.in_ = x.buf.tensor.data_ptr()
        d.dequant = 1.0 / self._scale(x) if self.dt == L.DT_FP8 else 1.0
        if nchw:
            d.out_c_off, d.out_c_stride, d.out_layout = 0, x.c, L.OUT_NCHW_F32
            op.out = self._val_ptr(out, idx, 'out')
        else:
            d.out_c_off, d.out_c_stride, d.out_layout = off, out.buf.c, L.OUT_NHWC
            op.out = out.buf.tensor.data_ptr()
        op.d.copy = d
        isz = self.dtype.itemsize
        nbytes = x.n * x.h * x.w * x.c * (isz + (4 if nchw else isz * scale * scale))
        self.op_info.append(dict(kind='copy', name='upsample2x' if scale == 2 else 'copy', flops=0, bytes=nbytes))
        return op

    # ------------------------------------------------------------------
    def _alloc_outputs(self):
        # fp32 NCHW heads; a classify node's output is [n][c2] (Flatten, nets/common.py:825)
        outs = [torch.empty((v.n, v.c) if v.producer.kind == 'classify' else (v.n, v.c, v.h, v.w),
                            dtype=torch.float32, device=self.device) for v in self.out_vals]
        self._bind_outputs(outs)
        return outs

    def _bind_outputs(self, outs):
        for v, t in zip(self.out_vals, outs):
            for idx, field in self.output_slots.get(id(v), []):
                setattr(self.ops[idx], field, None if idx in self.head_unstored else t.data_ptr())

    # ---- fused Detect heads (decode + candidate filter in the head conv) ----
    def head_ops(self):
        """Op index of each output's producing conv, when every output is a bf16 or
        e4m3 Detect-head 1x1 conv the fused kernels cover (ycx_conv2d_head), else None."""
        if self.dt == L.DT_F32:
            return None
        f8 = self.dt == L.DT_FP8
        idx = []
        for v in self.out_vals:
            slots = self.output_slots.get(id(v), [])
            if len(slots) != 1 or slots[0][1] != 'out':
                return None
            op = self.ops[slots[0][0]]
            d = op.d.conv
            if not (op.kind == L.OP_CONV and d.kh == 1 and d.kw == 1 and d.stride == 1 and d.pad == 0 and
                    d.act == L.ACT_NONE and d.out_layout == L.OUT_NCHW_F32 and d.cout <= 256 and
                    d.cin % (128 if f8 else 64) == 0 and d.in_c_off % (16 if f8 else 8) == 0 and
                    d.in_c_stride % (16 if f8 else 8) == 0):
                return None
            idx.append(slots[0][0])
        return idx

    def enable_head_decode(self, head_descs, cand, cand_rows, counts, keep_heads=True, status=None):
        """Turn the Detect-head convs into ycx_conv2d_head ops (decode_box + the
        candidate filter of detect.py:29-121 in the conv epilogue; candidates
        appended to cand / cand_rows / counts, which the caller zeroes before
        every forward). keep_heads: also store the raw fp32 NCHW logits.
        status: an int32 device tensor the head kernels set to
        YCX_HEAD_NONFINITE when a logit is inf / NaN (the fp16 range guard).
        Must precede capture(). Returns False when the plan does not qualify."""
        if self.graph_exec is not None:
            raise RuntimeError("ycx: enable_head_decode() after capture()")
        idx = self.head_ops()
        if idx is None or len(head_descs) != len(idx):
            return False
        for i, hd in zip(idx, head_descs):
            op = self.ops[i]
            conv = L.ConvDesc()
            ctypes.pointer(conv)[0] = op.d.conv
            if conv.cout_pad != 256:  # the head tile covers 256 output channels: zero-pad the weight rows
                wi = next(j for j, t in enumerate(self.params) if t.data_ptr() == op.weight)
                w, b = self.params[wi], self.params[wi + 1]
                w2 = torch.zeros((256,) + tuple(w.shape[1:]), dtype=w.dtype, device=w.device)
                if self.dt == L.DT_FP8:  # bias then dq, each [cout_pad]
                    b2 = torch.zeros((512,), dtype=b.dtype, device=b.device)
                    b2[:conv.cout] = b[:conv.cout]
                    b2[256:256 + conv.cout] = b[conv.cout_pad:conv.cout_pad + conv.cout]
                else:
                    b2 = torch.zeros((256,), dtype=b.dtype, device=b.device)
                    b2[:conv.cout] = b[:conv.cout]
                w2[:conv.cout] = w[:conv.cout]
                self.head_params += [w2, b2]   # self.params keeps the plan's shapes (prepack)
                op.weight, op.bias, conv.cout_pad = w2.data_ptr(), b2.data_ptr(), 256
            op.kind = L.OP_HEAD
            op.d.head.conv = conv
            op.d.head.head = hd
            op.cand, op.cand_rows, op.cand_counts = cand.data_ptr(), cand_rows.data_ptr(), counts.data_ptr()
            op.status = status.data_ptr() if status is not None else None
            tile = 39 if self.dt == L.DT_FP8 else 38
            self.op_info[i] = dict(self.op_info[i], name=L.lib.ycx_conv_tile_name(tile).decode(), kind='head')
            if not keep_heads:  # the logits never reach HBM (the candidates appended are ~KB)
                self.head_unstored.add(i)
                info = self.op_info[i]
                self.op_info[i] = dict(info, bytes=info['bytes'] - info.get('out_bytes', 0), out_bytes=0)
        if self.fixed_outputs is not None:
            self._bind_outputs(self.fixed_outputs)
        return True

    def _bind_input(self, x):
        if x.device != self.device or x.dtype != torch.float32 or not x.is_contiguous():
            x = x.to(self.device, torch.float32).contiguous()
        if tuple(x.shape) != self.shape:
            raise ValueError(f"ycx: engine built for {self.shape}, got {tuple(x.shape)}")
        for idx, field in self.input_slots:
            setattr(self.ops[idx], field, x.data_ptr())
        return x

    def _result(self, outs):
        return outs if self.is_list else outs[0]

    def run(self, x, events=None):
        """Eager forward: fresh output tensors every call (like the reference)."""
        x = self._bind_input(x)
        outs = self._alloc_outputs()
        self._static_bound = False  # the op array now points at this call's tensors
        ev = None
        if events is not None:
            ev = (ctypes.c_void_p * (self.n_ops + 1))(*[e.cuda_event for e in events])
        stream = L.stream_handle(self.device)
        L.check(L.lib.ycx_run_ops(self.ops, self.n_ops, stream, ev), "ycx_run_ops")
        return self._result(outs)

    # ---- static-I/O path for benchmarking / serving loops ----
    def bind_static(self, x):
        """Pin the plan to persistent input/output tensors (required by capture()).
        Idempotent: every caller of one engine shares the same static tensors
        (and the HIP graph captured on them)."""
        if self.fixed_outputs is None:
            self.static_input = self._bind_input(x)
            self.fixed_outputs = self._alloc_outputs()
            self._static_bound = True
        return self.static_input, self._result(self.fixed_outputs)

    def _ensure_static(self):
        if not self._static_bound:  # an eager run() re-pointed the op array
            self._bind_input(self.static_input)
            self._bind_outputs(self.fixed_outputs)
            self._static_bound = True

    def run_static(self, events=None):
        self._ensure_static()
        ev = None
        ops, n_ops = self.ops, self.n_ops
        if events is not None:  # per-op events: the plan's own op list
            ev = (ctypes.c_void_p * (self.n_ops + 1))(*[e.cuda_event for e in events])
        else:
            ops, n_ops = self._exec_ops()
        L.check(L.lib.ycx_run_ops(ops, n_ops, L.stream_handle(self.device), ev), "ycx_run_ops")
        return self._result(self.fixed_outputs)

    # ---- image-chunked prefix (experiment: keep the memory-bound high-resolution layers'
    # working set in the 256 MiB Infinity Cache by running them k images at a time) ----
    def _esize(self):
        return {L.DT_BF16: 2, L.DT_F16: 2, L.DT_F32: 4, L.DT_FP8: 1}[self.dt]

    def _chunk_op(self, op, i0, k):
        """A copy of ``op`` restricted to images [i0, i0 + k): every operand is image-major,
        so the restriction is n = k and a pointer offset per operand."""
        o = L.Op()
        ctypes.pointer(o)[0] = op
        es = self._esize()

        def shift(field, per_image):
            v = getattr(o, field)
            if v:
                setattr(o, field, v + i0 * per_image)

        if o.kind in (L.OP_CONV, L.OP_STEM, L.OP_STEM2, L.OP_STEM_REORG, L.OP_GCONV, L.OP_DECONV, L.OP_GHOST):
            d = o.d.pair[1] if o.kind == L.OP_STEM2 else o.d.conv
            first = o.d.pair[0] if o.kind == L.OP_STEM2 else d
            if o.kind in (L.OP_CONV, L.OP_GCONV, L.OP_DECONV, L.OP_GHOST):
                shift('in_', (4 if d.in_pool else 1) * d.h * d.w * d.in_c_stride * es)
            else:  # fp32 NCHW image
                shift('in_', first.cin * first.h * first.w * 4)
            if d.out_layout == L.OUT_NCHW_F32:
                shift('out', d.out_c_stride * d.ho * d.wo * 4)
            else:
                shift('out', (4 if d.out_layout == L.OUT_NHWC_UP2 else 1) * d.ho * d.wo * d.out_c_stride * es)
            shift('residual', d.ho * d.wo * d.res_c_stride * es)
            for dd in ((o.d.pair[0], o.d.pair[1]) if o.kind == L.OP_STEM2 else (o.d.conv,)):
                dd.n = k
        elif o.kind == L.OP_POOL:
            d = o.d.pool
            shift('in_', d.h * d.w * d.in_c_stride * es)
            shift('out', d.ho * d.wo * d.out_c_stride * es)
            d.n = k
        elif o.kind == L.OP_DEPTH:
            d = o.d.depth
            shift('in_', d.h * d.w * d.in_c_stride * es)
            shift('out', d.ho * d.wo * d.out_c_stride * es)
            d.n = k
        elif o.kind == L.OP_COPY:
            d = o.d.copy
            shift('in_', d.h * d.w * d.in_c_stride * es)
            if d.out_layout == L.OUT_NCHW_F32:
                shift('out', d.out_c_stride * d.h * d.w * 4)
            else:
                shift('out', d.scale * d.scale * d.h * d.w * d.out_c_stride * es)
            d.n = k
        else:
            raise ValueError("ycx: cannot chunk this op kind")
        return o

    @staticmethod
    def _op_out_h(op):
        if op.kind in (L.OP_CONV, L.OP_STEM, L.OP_HEAD, L.OP_STEM_REORG, L.OP_GCONV, L.OP_DECONV, L.OP_GHOST):
            return op.d.conv.ho
        if op.kind == L.OP_STEM2:
            return op.d.pair[1].ho
        if op.kind == L.OP_POOL:
            return op.d.pool.ho
        if op.kind == L.OP_DEPTH:
            return op.d.depth.ho
        if op.kind == L.OP_CLASSIFY:
            return 1
        return op.d.copy.h * op.d.copy.scale

    def _exec_ops(self):
        """The op array a forward runs: the plan, or with YCX_CHUNK='k:cut' its first ``cut``
        ops run k images at a time (all of them for images 0..k-1, then k..2k-1, ...)."""
        spec = os.environ.get('YCX_CHUNK')
        n = self.shape[0]
        if not spec:
            return self.ops, self.n_ops
        ks, cs = spec.split(':')
        k = int(ks)
        if cs.startswith('@'):  # '@H': every op up to the first whose output is below H rows
            hmin, cut = int(cs[1:]), 0
            while cut < self.n_ops and self._op_out_h(self.ops[cut]) >= hmin:
                cut += 1
        else:
            cut = min(int(cs), self.n_ops)
        if k <= 0 or k >= n or n % k or any(self.ops[i].kind == L.OP_HEAD for i in range(cut)):
            return self.ops, self.n_ops
        ops = [self._chunk_op(self.ops[i], i0, k) for i0 in range(0, n, k) for i in range(cut)]
        ops += [self.ops[i] for i in range(cut, self.n_ops)]
        self._chunked_ops = (L.Op * len(ops))(*ops)
        return self._chunked_ops, len(ops)

    def capture(self):
        """Capture the static plan into a HIP graph (one launch per forward)."""
        if self.fixed_outputs is None:
            raise RuntimeError("ycx: call bind_static() before capture()")
        if self.graph_exec is None:
            self._ensure_static()
            h = ctypes.c_void_p()
            s = torch.cuda.Stream(self.device)
            s.wait_stream(torch.cuda.current_stream(self.device))
            ops, n_ops = self._exec_ops()
            L.check(L.lib.ycx_graph_capture(ops, n_ops, s.cuda_stream, ctypes.byref(h)),
                    "ycx_graph_capture")
            torch.cuda.current_stream(self.device).wait_stream(s)
            self.graph_exec = h.value
        return self.graph_exec

    def replay(self):
        L.check(L.lib.ycx_graph_launch(self.graph_exec, L.stream_handle(self.device)), "ycx_graph_launch")
        return self._result(self.fixed_outputs)

    def close(self):
        if self.graph_exec is not None:
            L.lib.ycx_graph_destroy(self.graph_exec)
            self.graph_exec = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- introspection ----
    @property
    def flops_per_image(self):
        return self.conv_flops / self.shape[0]

    def summary(self):
        kinds = {}
        for info in self.op_info:
            kinds[info['kind']] = kinds.get(info['kind'], 0) + 1
        mem = sum(t.numel() * t.element_size() for t in self.buffers)
        return dict(ops=self.n_ops, kinds=kinds, activation_bytes=mem, gflop_per_image=self.flops_per_image / 1e9)
