"""The shared RobustConv2 test network ("rc2-mini"): a Conv stem to 32 channels, the three RobustConv2
forms the reference's own comment recommends -- [32, 5, 2], [32, 7, 4], [32, 11, 8]: a depthwise conv
of stride 2 / 4 / 8 and the transposed conv (kernel == stride) that restores the resolution -- as
parallel paths next to a plain 1x1 path, all four written straight into the slices of one concat
buffer, then two Convs and a two-level IDetect head.
tests/golden/make_golden_rc2.py records the reference's outputs for it (g8_rc2.npz / .json).

Weights: ycx.utils.synth knows neither nn.ConvTranspose2d nor RobustConv2's layer scale (it keeps the
tensors it does not know, here an unseeded init and gamma = 1e-6, which would scale every RobustConv2
output below any tolerance), so ``state_dict`` seeds those three tensors itself, gamma at O(1)."""
import numpy as np
import torch

from ycx.utils.synth import normal, synthetic_state_dict, tensor_seed

NC = 3
ANCHORS2 = [[10, 13, 16, 30, 33, 23], [30, 61, 62, 45, 59, 119]]  # two levels, 3 anchors each
SHAPE = (2, 3, 64, 64)
IMG_SEED, W_SEED = 800, 29
STRIDES = [2.0, 4.0]
OUT_LAYERS = [6, 7]
RC2 = [(5, 2), (7, 4), (11, 8)]  # (k, s) of layers 1, 2, 3

_BACKBONE = [
    [-1, 1, 'Conv', [32, 3, 1]],            # 0   32 @ 64
    [0, 1, 'RobustConv2', [32, 5, 2]],      # 1   32 @ 64  depthwise k5 s2 -> 32, deconv x2
    [0, 1, 'RobustConv2', [32, 7, 4]],      # 2   32 @ 64  depthwise k7 s4 -> 16, deconv x4
    [0, 1, 'RobustConv2', [32, 11, 8]],     # 3   32 @ 64  depthwise k11 s8 -> 8, deconv x8
    [0, 1, 'Conv', [32, 1, 1]],             # 4   32 @ 64
    [[1, 2, 3, 4], 1, 'Concat', [1]],       # 5  128 @ 64
    [-1, 1, 'Conv', [128, 3, 2]],           # 6  128 @ 32
]
_HEAD = [
    [-1, 1, 'Conv', [128, 3, 2]],           # 7  128 @ 16
]


def _copy(rows):
    return [[list(f) if isinstance(f, list) else f, n, m, list(a)] for f, n, m, a in rows]


def rc2_mini():
    return {'depth_multiple': 1.0, 'width_multiple': 1.0, 'backbone': _copy(_BACKBONE),
            'head': _copy(_HEAD) + [[list(OUT_LAYERS), 1, 'IDetect', ['nc', 'anchors']]]}


def state_dict(model, seed=W_SEED):
    """synthetic_state_dict plus the tensors it keeps: conv_deconv.weight ~ N(0, 2 / cin) (each output
    sums cin products), conv_deconv.bias ~ 0.1 N, gamma ~ 1 + 0.25 N."""
    sd = synthetic_state_dict(model, seed=seed)
    for key, t in sd.items():
        s, n = tensor_seed(seed, key), t.numel()
        if key.endswith('conv_deconv.weight'):
            v = normal(s, n) * np.sqrt(2.0 / t.shape[0])
        elif key.endswith('conv_deconv.bias'):
            v = 0.1 * normal(s, n)
        elif key.endswith('.gamma'):
            v = 1.0 + 0.25 * normal(s, n)
        else:
            continue
        sd[key] = torch.from_numpy(v.reshape(tuple(t.shape))).to(t.dtype)
    return sd
