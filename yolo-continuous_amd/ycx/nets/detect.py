"""Detection heads as parameter holders (lowered to HIP convs by the engine).

Detect  — nets/detect.py:4-38: three 1x1 convs with bias; eval returns the raw
          logits [P5, P4, P3] (NCHW fp32), no decode.
IDetect — nets/idetect.py:7-50: ImplicitA -> 1x1 conv -> ImplicitM, reshaped to
          (bs, na, ny, nx, no); in eval also the decoded boxes in pixels. The
          reference leaves ``stride`` as None so its eval raises TypeError
          (SURVEY.md Appendix B.7); here the strides default to
          image_size / ny per level (documented deviation).
IAuxDetect — nets/iaux_detect.py:7-49: IDetect's main heads on x[:nl] plus
          auxiliary 1x1 heads ``m2`` on x[nl:]. Eval returns
          (cat(z, 1), x[:nl]): the aux maps are computed and discarded
          (:32-33, :49), so the engine lowers only the main heads and the aux
          branch is dead code it never launches.
IBin    — nets/ibin.py:8-74: IDetect's head at the width nc + 3 + 2 * (bin_count + 1); in eval
          width and height are decoded by SigmoidBin.forward (losses/sigmoid_bin.py:49-63): the
          centre of the best of 21 bins plus a regression term, clamped to [0, 4], times the anchor.
"""
from __future__ import annotations

import warnings

import torch
from torch import nn

from .common import ImplicitA, ImplicitM, _Holder


class Detect(_Holder):
    def __init__(self, num_classes=80, anchors=(), ch=()):
        super().__init__()
        self.num_classes = num_classes
        self.len_output = num_classes + 5
        self.num_layers = len(anchors)
        self.num_anchors_each_layer = len(anchors[0]) // 2
        out_c = self.num_anchors_each_layer * self.len_output
        # Attribute names = state_dict keys of the reference (model.N.yolo_head_P*).
        self.yolo_head_P3 = nn.Conv2d(ch[0], out_c, 1)
        self.yolo_head_P4 = nn.Conv2d(ch[1], out_c, 1)
        self.yolo_head_P5 = nn.Conv2d(ch[2], out_c, 1)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, 0, 0.01)

    def heads_in_output_order(self):
        """(conv, input position) pairs in the order the reference returns them."""
        return [(self.yolo_head_P5, 2), (self.yolo_head_P4, 1), (self.yolo_head_P3, 0)]


class IDetect(_Holder):
    stride = None

    def __init__(self, nc=80, anchors=(), ch=()):
        super().__init__()
        self.nc = nc
        self.no = nc + 5
        self.nl = len(anchors)
        self.na = len(anchors[0]) // 2
        a = torch.tensor(anchors).float().view(self.nl, -1, 2)
        self.register_buffer('anchors', a)
        self.register_buffer('anchor_grid', a.clone().view(self.nl, 1, -1, 1, 1, 2))
        self.m = nn.ModuleList(nn.Conv2d(x, self.no * self.na, 1) for x in ch)
        self.ia = nn.ModuleList(ImplicitA(x) for x in ch)
        self.im = nn.ModuleList(ImplicitM(self.no * self.na) for _ in ch)


class SigmoidBin(_Holder):
    """The buffers of losses/sigmoid_bin.py:6-44 that IBin's eval reads or its state_dict lists:
    ``bins`` (the bin centres, :33-38) and ``BCE_bins.pos_weight`` (:43). ``step`` is the
    regression term's scale (:35, :51). No loss is implemented."""

    def __init__(self, bin_count=10, min=0.0, max=1.0, bce_weight=1.0):
        super().__init__()
        self.bin_count, self.length = bin_count, bin_count + 1
        self.min, self.max = min, max
        self.scale = float(max - min)
        start = min + (self.scale / 2.0) / bin_count
        end = max - (self.scale / 2.0) / bin_count
        self.step = step = self.scale / bin_count
        with warnings.catch_warnings():  # torch.range is deprecated; its end-inclusive values are the schema
            warnings.simplefilter('ignore')
            bins = torch.range(start, end + 0.0001, step).float()
        assert bins.numel() == bin_count, (bins.numel(), bin_count)
        self.register_buffer('bins', bins)
        self.BCE_bins = nn.BCEWithLogitsLoss(pos_weight=torch.Tensor([bce_weight]))

    def get_length(self):
        return self.length


class IBin(_Holder):
    """Schema of nets/ibin.py:8-33: IDetect's convs and implicit layers at the width
    no = nc + 3 + 2 * (bin_count + 1) (x, y, objectness, and for w and for h one regression logit
    plus bin_count bin logits), and the two SigmoidBin children whose ``bins`` the eval decode
    reads. A sibling of IDetect, not a subclass: its eval branch is another kernel
    (ycx_ibin_decode). The reference's eval slices are written out for 21 bins (:62-70), so any
    other bin_count is refused."""
    stride = None

    def __init__(self, nc=80, anchors=(), ch=(), bin_count=21):
        super().__init__()
        if bin_count != 21:
            raise NotImplementedError(f"ycx: IBin with bin_count={bin_count}: the reference's eval branch slices "
                                      f"its output for bin_count == 21 only (nets/ibin.py:62-70)")
        self.nc = nc
        self.bin_count = bin_count
        self.w_bin_sigmoid = SigmoidBin(bin_count=bin_count, min=0.0, max=4.0)
        self.h_bin_sigmoid = SigmoidBin(bin_count=bin_count, min=0.0, max=4.0)
        self.no = nc + 3 + self.w_bin_sigmoid.get_length() + self.h_bin_sigmoid.get_length()
        self.nl = len(anchors)
        self.na = len(anchors[0]) // 2
        a = torch.tensor(anchors).float().view(self.nl, -1, 2)
        self.register_buffer('anchors', a)
        self.register_buffer('anchor_grid', a.clone().view(self.nl, 1, -1, 1, 1, 2))
        self.m = nn.ModuleList(nn.Conv2d(x, self.no * self.na, 1) for x in ch)
        self.ia = nn.ModuleList(ImplicitA(x) for x in ch)
        self.im = nn.ModuleList(ImplicitM(self.no * self.na) for _ in ch)


class IAuxDetect(IDetect):
    """Schema of nets/iaux_detect.py:11-25 (state_dict keys anchors, anchor_grid,
    m.*, m2.*, ia.*, im.*). ``ch`` lists the main inputs then the aux inputs."""

    def __init__(self, nc=80, anchors=(), ch=()):
        nl = len(anchors)
        super().__init__(nc, anchors, ch[:nl])
        self.m2 = nn.ModuleList(nn.Conv2d(x, self.no * self.na, 1) for x in ch[nl:])
