"""Layer modules of the YOLOv7 graph, as parameter holders for the HIP engine.

Each class keeps the constructor signature and the parameter/buffer attribute
names of the reference module it stands for, so a reference ``state_dict``
(e.g. the 558-key yolov7 schema) loads unchanged. The modules
hold no ``forward`` compute: ``Model.forward`` lowers the whole module tree to
a static plan of HIP kernels (``ycx.engine``), folding BatchNorm, RepConv
branches and ImplicitA/M into conv weight/bias on the way.

Reference: nets/common.py (line numbers cited per class).
"""
from __future__ import annotations

import math

import torch
from torch import nn


def autopad(k, p=None):
    """'same' padding for odd kernels (nets/common.py:7-11)."""
    if p is None:
        p = k // 2 if isinstance(k, int) else [x // 2 for x in k]
    return p


class _Holder(nn.Module):
    """Base: calling a layer module directly is not a compute path."""

    def forward(self, *args, **kwargs):  # pragma: no cover - guard
        raise RuntimeError(f"ycx: {type(self).__name__} is lowered by Model.forward into HIP kernels; "
                           f"call the Model, not the layer")


class Conv(_Holder):
    """act(bn(conv2d(x))), bias-free conv, BN eps 1e-5 (nets/common.py:97-109)."""

    def __init__(self, c1, c2, k=1, s=1, p=None, g=1, act=True):
        super().__init__()
        self.conv = nn.Conv2d(c1, c2, k, s, autopad(k, p), groups=g, bias=False)
        self.bn = nn.BatchNorm2d(c2)
        self.act = nn.SiLU() if act is True else (act if isinstance(act, nn.Module) else nn.Identity())


def dw_conv(c1, c2, k=1, s=1, act=True):
    """Depthwise Conv: groups = gcd(c1, c2) (nets/common.py:20-22); a function there too."""
    return Conv(c1, c2, k, s, g=math.gcd(c1, c2), act=act)


class RobustConv(_Holder):
    """conv1x1(conv_dw(x)) * gamma: a depthwise k x k Conv, a biased 1x1 conv and a learned
    per-channel layer scale (nets/common.py:112-124). The engine folds gamma into the 1x1."""

    def __init__(self, c1, c2, k=7, s=1, p=None, g=1, act=True, layer_scale_init_value=1e-6):
        super().__init__()
        self.conv_dw = Conv(c1, c1, k=k, s=s, p=p, g=c1, act=act)
        self.conv1x1 = nn.Conv2d(c1, c2, 1, 1, 0, groups=1, bias=True)
        self.gamma = nn.Parameter(layer_scale_init_value * torch.ones(c2)) if layer_scale_init_value > 0 else None


class RobustConv2(_Holder):
    """conv_deconv(conv_strided(x)) * gamma: a depthwise k x k Conv of stride s, a biased transposed
    conv with kernel == stride == s that restores the resolution, and a learned per-channel layer scale
    (nets/common.py:127-139; its comment recommends [32, 5, 2], [32, 7, 4] or [32, 11, 8]). The engine
    folds gamma into the transposed conv (ycx_deconv2d)."""

    def __init__(self, c1, c2, k=7, s=4, p=None, g=1, act=True, layer_scale_init_value=1e-6):
        super().__init__()
        self.conv_strided = Conv(c1, c1, k=k, s=s, p=p, g=c1, act=act)
        self.conv_deconv = nn.ConvTranspose2d(in_channels=c1, out_channels=c2, kernel_size=s, stride=s, padding=0,
                                              bias=True, dilation=1, groups=1)
        self.gamma = nn.Parameter(layer_scale_init_value * torch.ones(c2)) if layer_scale_init_value > 0 else None


class GhostConv(_Holder):
    """cat[y, cv2(y)] with y = cv1(x): a Conv to half the channels and a depthwise 5x5 / s1 Conv on its
    output (nets/common.py:142-152). The engine runs cv2, the concat and Ghost's shortcut as one
    ycx_ghost_dw launch."""

    def __init__(self, c1, c2, k=1, s=1, g=1, act=True):
        super().__init__()
        c_ = c2 // 2
        self.cv1 = Conv(c1, c_, k, s, None, g, act)
        self.cv2 = Conv(c_, c_, 5, 1, None, c_, act)


class Ghost(_Holder):
    """conv(x) + shortcut(x): GhostConv, a depthwise k x k / s2 Conv when s == 2, GhostConv without
    activation; the shortcut is the identity, or for s == 2 a depthwise Conv and a 1x1 Conv, both
    without activation (nets/common.py:233-245)."""

    def __init__(self, c1, c2, k=3, s=1):
        super().__init__()
        c_ = c2 // 2
        self.conv = nn.Sequential(GhostConv(c1, c_, 1, 1),
                                  dw_conv(c_, c_, k, s, act=False) if s == 2 else nn.Identity(),
                                  GhostConv(c_, c2, 1, 1, act=False))
        self.shortcut = nn.Sequential(dw_conv(c1, c1, k, s, act=False),
                                      Conv(c1, c2, 1, 1, act=False)) if s == 2 else nn.Identity()


class MP(_Holder):
    """MaxPool2d(k, k) (nets/common.py:25-31)."""

    def __init__(self, k=2):
        super().__init__()
        self.m = nn.MaxPool2d(kernel_size=k, stride=k)


class SP(_Holder):
    """MaxPool2d(k, s, k//2) (nets/common.py:34-40)."""

    def __init__(self, k=3, s=1):
        super().__init__()
        self.m = nn.MaxPool2d(kernel_size=k, stride=s, padding=k // 2)


class ReOrg(_Holder):
    """Space-to-depth x(b, c, 2h, 2w) -> (b, 4c, h, w): cat of the (even, even), (odd, even),
    (even, odd), (odd, odd) row / column samples (nets/common.py:43-51). No parameters; the
    engine folds it into the operand gather of the Conv that reads it (ycx_stem_conv_reorg)."""


class Focus(_Holder):
    """conv(cat of the four pixel phases of x), x(b, c, 2h, 2w) -> (b, c2, h, w): the phases in ReOrg's
    order, then a Conv(4 c1, c2, k, s, p, g, act) (nets/common.py:759-767). On the image the engine
    folds the regrouping into that conv's gather (ycx_stem_conv_reorg); on an activation it runs
    ycx_space_depth in focus mode."""

    def __init__(self, c1, c2, k=1, s=1, p=None, g=1, act=True):
        super().__init__()
        self.conv = Conv(c1 * 4, c2, k, s, p, g, act)


class Contract(_Holder):
    """Width-height into channels, x(b, c, h, w) -> (b, c s^2, h/s, w/s), channel (a s + b) c + i from
    pixel phase (a, b) (nets/common.py:787-798). No parameters; ycx_space_depth."""

    def __init__(self, gain=2):
        super().__init__()
        self.gain = gain


class Expand(_Holder):
    """Channels into width-height, x(b, c, h, w) -> (b, c / s^2, h s, w s), Contract's inverse
    (nets/common.py:801-812). No parameters; ycx_space_depth."""

    def __init__(self, gain=2):
        super().__init__()
        self.gain = gain


class Concat(_Holder):
    """Channel concat (nets/common.py:54-60); never materialised on device."""

    def __init__(self, dimension=1):
        super().__init__()
        self.d = dimension


class Bottleneck(_Holder):
    """x + cv2(cv1(x)) when shortcut and c1 == c2 (nets/common.py:199-209)."""

    def __init__(self, c1, c2, shortcut=True, g=1, e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c_, c2, 3, 1, g=g)
        self.add = shortcut and c1 == c2


class Res(_Holder):
    """x + cv3(cv2(cv1(x))) when shortcut and c1 == c2, cv2 a (grouped) 3x3 (nets/common.py:212-223)."""

    def __init__(self, c1, c2, shortcut=True, g=1, e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c_, c_, 3, 1, g=g)
        self.cv3 = Conv(c_, c2, 1, 1)
        self.add = shortcut and c1 == c2


class ResX(Res):
    """Res with 32 groups (nets/common.py:226-230)."""

    def __init__(self, c1, c2, shortcut=True, g=32, e=0.5):
        super().__init__(c1, c2, shortcut, g, e)


class DownC(_Holder):
    """cat[cv2(cv1 x), cv3(maxpool_k x)]: the P6 down-sampling block (nets/common.py:171-182)."""

    def __init__(self, c1, c2, n=1, k=2):
        super().__init__()
        c_ = int(c1)
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c_, c2 // 2, 3, k)
        self.cv3 = Conv(c1, c2 // 2, 1, 1)
        self.mp = nn.MaxPool2d(kernel_size=k, stride=k)


class SPP(_Holder):
    """cv2(cat[x, mp5, mp9, mp13](cv1 x)) (nets/common.py:185-196)."""

    def __init__(self, c1, c2, k=(5, 9, 13)):
        super().__init__()
        c_ = c1 // 2
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c_ * (len(k) + 1), c2, 1, 1)
        self.m = nn.ModuleList([nn.MaxPool2d(kernel_size=x, stride=1, padding=x // 2) for x in k])


class SPPCSPC(_Holder):
    """CSP spatial pyramid pooling block of yolov7 layer 51 (nets/common.py:248-266)."""

    def __init__(self, c1, c2, n=1, shortcut=False, g=1, e=0.5, k=(5, 9, 13)):
        super().__init__()
        c_ = int(2 * c2 * e)
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c1, c_, 1, 1)
        self.cv3 = Conv(c_, c_, 3, 1)
        self.cv4 = Conv(c_, c_, 1, 1)
        self.m = nn.ModuleList([nn.MaxPool2d(kernel_size=x, stride=1, padding=x // 2) for x in k])
        self.cv5 = Conv(4 * c_, c_, 1, 1)
        self.cv6 = Conv(c_, c_, 3, 1)
        self.cv7 = Conv(2 * c_, c2, 1, 1)


class GhostSPPCSPC(SPPCSPC):
    """SPPCSPC with every Conv a GhostConv (nets/common.py:269-280). Like the reference it builds the
    parent's plain convs first and then replaces them."""

    def __init__(self, c1, c2, n=1, shortcut=False, g=1, e=0.5, k=(5, 9, 13)):
        super().__init__(c1, c2, n, shortcut, g, e, k)
        c_ = int(2 * c2 * e)
        self.cv1 = GhostConv(c1, c_, 1, 1)
        self.cv2 = GhostConv(c1, c_, 1, 1)
        self.cv3 = GhostConv(c_, c_, 3, 1)
        self.cv4 = GhostConv(c_, c_, 1, 1)
        self.cv5 = GhostConv(4 * c_, c_, 1, 1)
        self.cv6 = GhostConv(c_, c_, 3, 1)
        self.cv7 = GhostConv(2 * c_, c2, 1, 1)


class BottleneckCSPA(_Holder):
    """cv3(cat[m(cv1 x), cv2 x]) (nets/common.py:294-307)."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c1, c_, 1, 1)
        self.cv3 = Conv(2 * c_, c2, 1, 1)
        self.m = nn.Sequential(*[Bottleneck(c_, c_, shortcut, g, e=1.0) for _ in range(n)])


class BottleneckCSPB(_Holder):
    """x1 = cv1 x; cv3(cat[m(x1), cv2 x1]) (nets/common.py:310-324)."""

    def __init__(self, c1, c2, n=1, shortcut=False, g=1, e=0.5):
        super().__init__()
        c_ = int(c2)
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c_, c_, 1, 1)
        self.cv3 = Conv(2 * c_, c2, 1, 1)
        self.m = nn.Sequential(*[Bottleneck(c_, c_, shortcut, g, e=1.0) for _ in range(n)])


class BottleneckCSPC(_Holder):
    """cv4(cat[cv3(m(cv1 x)), cv2 x]) (nets/common.py:327-341)."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c1, c_, 1, 1)
        self.cv3 = Conv(c_, c_, 1, 1)
        self.cv4 = Conv(2 * c_, c2, 1, 1)
        self.m = nn.Sequential(*[Bottleneck(c_, c_, shortcut, g, e=1.0) for _ in range(n)])


class ResCSPA(BottleneckCSPA):
    """BottleneckCSPA over Res blocks (nets/common.py:344-349)."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        self.m = nn.Sequential(*[Res(c_, c_, shortcut, g, e=0.5) for _ in range(n)])


class ResCSPB(BottleneckCSPB):
    """BottleneckCSPB over Res blocks (nets/common.py:352-357)."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2)
        self.m = nn.Sequential(*[Res(c_, c_, shortcut, g, e=0.5) for _ in range(n)])


class ResCSPC(BottleneckCSPC):
    """BottleneckCSPC over Res blocks (nets/common.py:360-365)."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        self.m = nn.Sequential(*[Res(c_, c_, shortcut, g, e=0.5) for _ in range(n)])


class ResXCSPA(ResCSPA):
    """ResCSPA with 32 groups and e = 1 inner blocks (nets/common.py:368-373)."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=32, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        self.m = nn.Sequential(*[Res(c_, c_, shortcut, g, e=1.0) for _ in range(n)])


class ResXCSPB(ResCSPB):
    """ResCSPB with 32 groups and e = 1 inner blocks (nets/common.py:376-381)."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=32, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2)
        self.m = nn.Sequential(*[Res(c_, c_, shortcut, g, e=1.0) for _ in range(n)])


class ResXCSPC(ResCSPC):
    """ResCSPC with 32 groups and e = 1 inner blocks (nets/common.py:384-389)."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=32, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        self.m = nn.Sequential(*[Res(c_, c_, shortcut, g, e=1.0) for _ in range(n)])


class GhostCSPA(BottleneckCSPA):
    """BottleneckCSPA over Ghost blocks (nets/common.py:392-397)."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        self.m = nn.Sequential(*[Ghost(c_, c_) for _ in range(n)])


class GhostCSPB(BottleneckCSPB):
    """BottleneckCSPB over Ghost blocks (nets/common.py:400-405)."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2)
        self.m = nn.Sequential(*[Ghost(c_, c_) for _ in range(n)])


class GhostCSPC(BottleneckCSPC):
    """BottleneckCSPC over Ghost blocks (nets/common.py:408-413)."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        self.m = nn.Sequential(*[Ghost(c_, c_) for _ in range(n)])


class ImplicitA(_Holder):
    """Learned additive channel bias (nets/common.py:416-426)."""

    def __init__(self, channel, mean=0., std=.02):
        super().__init__()
        import torch
        self.channel, self.mean, self.std = channel, mean, std
        self.implicit = nn.Parameter(torch.zeros(1, channel, 1, 1))
        nn.init.normal_(self.implicit, mean=self.mean, std=self.std)


class ImplicitM(_Holder):
    """Learned multiplicative channel scale (nets/common.py:429-439)."""

    def __init__(self, channel, mean=0., std=.02):
        super().__init__()
        import torch
        self.channel, self.mean, self.std = channel, mean, std
        self.implicit = nn.Parameter(torch.ones(1, channel, 1, 1))
        nn.init.normal_(self.implicit, mean=self.mean, std=self.std)


class RepConv(_Holder):
    """RepVGG block: act(BN(conv3x3) + BN(conv1x1) [+ BN(x)]) (nets/common.py:442-486).

    The engine always runs the re-parameterised single 3x3 conv; the branch
    folding restates get_equivalent_kernel_bias / _fuse_bn_tensor
    (nets/common.py:488-529)."""

    def __init__(self, c1, c2, k=3, s=1, p=None, g=1, act=True, deploy=False):
        super().__init__()
        assert k == 3
        assert autopad(k, p) == 1
        self.deploy = deploy
        self.groups = g
        self.in_channels = c1
        self.out_channels = c2
        self.stride = s
        padding_11 = autopad(k, p) - k // 2
        self.act = nn.SiLU() if act is True else (act if isinstance(act, nn.Module) else nn.Identity())
        if deploy:
            self.rbr_reparam = nn.Conv2d(c1, c2, k, s, autopad(k, p), groups=g, bias=True)
        else:
            self.rbr_identity = nn.BatchNorm2d(num_features=c1) if c2 == c1 and s == 1 else None
            self.rbr_dense = nn.Sequential(nn.Conv2d(c1, c2, k, s, autopad(k, p), groups=g, bias=False),
                                           nn.BatchNorm2d(num_features=c2))
            self.rbr_1x1 = nn.Sequential(nn.Conv2d(c1, c2, 1, s, padding_11, groups=g, bias=False),
                                         nn.BatchNorm2d(num_features=c2))


class RepBottleneck(Bottleneck):
    """Bottleneck with cv2 a RepConv (nets/common.py:617-622). Like the reference it builds the parent with
    shortcut=True, g=1, e=0.5 whatever it was given (so cv1 emits c2 / 2 channels and ``add`` ignores
    ``shortcut``) and then sizes the RepConv from the ``e`` it was given: only e == 0.5 runs."""

    def __init__(self, c1, c2, shortcut=True, g=1, e=0.5):
        super().__init__(c1, c2, shortcut=True, g=1, e=0.5)
        c_ = int(c2 * e)
        self.cv2 = RepConv(c_, c2, 3, 1, g=g)


class RepRes(Res):
    """Res with cv2 a RepConv (nets/common.py:649-654)."""

    def __init__(self, c1, c2, shortcut=True, g=1, e=0.5):
        super().__init__(c1, c2, shortcut, g, e)
        c_ = int(c2 * e)
        self.cv2 = RepConv(c_, c_, 3, 1, g=g)


class RepResCSPA(ResCSPA):
    """ResCSPA over RepRes blocks (nets/common.py:657-662)."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        self.m = nn.Sequential(*[RepRes(c_, c_, shortcut, g, e=0.5) for _ in range(n)])


class RepResCSPB(ResCSPB):
    """ResCSPB over RepRes blocks (nets/common.py:665-670)."""

    def __init__(self, c1, c2, n=1, shortcut=False, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2)
        self.m = nn.Sequential(*[RepRes(c_, c_, shortcut, g, e=0.5) for _ in range(n)])


class RepResCSPC(ResCSPC):
    """ResCSPC over RepRes blocks (nets/common.py:673-678)."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        self.m = nn.Sequential(*[RepRes(c_, c_, shortcut, g, e=0.5) for _ in range(n)])


class RepResX(ResX):
    """ResX with cv2 a grouped RepConv, 32 groups by default (nets/common.py:681-686)."""

    def __init__(self, c1, c2, shortcut=True, g=32, e=0.5):
        super().__init__(c1, c2, shortcut, g, e)
        c_ = int(c2 * e)
        self.cv2 = RepConv(c_, c_, 3, 1, g=g)


class RepResXCSPA(ResXCSPA):
    """ResXCSPA over RepResX blocks (nets/common.py:689-694)."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=32, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        self.m = nn.Sequential(*[RepResX(c_, c_, shortcut, g, e=0.5) for _ in range(n)])


class RepResXCSPB(ResXCSPB):
    """ResXCSPB over RepResX blocks (nets/common.py:697-702)."""

    def __init__(self, c1, c2, n=1, shortcut=False, g=32, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2)
        self.m = nn.Sequential(*[RepResX(c_, c_, shortcut, g, e=0.5) for _ in range(n)])


class RepResXCSPC(ResXCSPC):
    """ResXCSPC over RepResX blocks (nets/common.py:705-710)."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=32, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        self.m = nn.Sequential(*[RepResX(c_, c_, shortcut, g, e=0.5) for _ in range(n)])


class Classify(_Holder):
    """Classification head, x(b, c1, h, w) -> (b, c2): AdaptiveAvgPool2d(1), a biased Conv2d(c1, c2, k, s,
    autopad(k, p), groups=g) on the 1 x 1 map, Flatten (nets/common.py:815-825). The engine runs the pool
    and the conv's centre tap as one ycx_classify op."""

    def __init__(self, c1, c2, k=1, s=1, p=None, g=1):
        super().__init__()
        self.aap = nn.AdaptiveAvgPool2d(1)
        self.conv = nn.Conv2d(c1, c2, k, s, autopad(k, p), groups=g)
        self.flat = nn.Flatten()


class SPPF(_Holder):
    """cv2(cat[x, m x, m m x, m m m x]) with k=5 (nets/common.py:771-784)."""

    def __init__(self, c1, c2, k=5):
        super().__init__()
        c_ = c1 // 2
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c_ * 4, c2, 1, 1)
        self.m = nn.MaxPool2d(kernel_size=k, stride=1, padding=k // 2)
