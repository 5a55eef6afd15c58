"""The shared grouped-conv test network ("gx-mini"): depthwise and grouped convs of every group width
the grouped kernel takes (cin_g 1, 2, 4, 8 is exercised by the kernel test; here 1, 2, 4, 16), in the
blocks that carry them -- dw_conv, ResX, ResXCSPC, ResCSPA (dense 3x3 path), Bottleneck with g = 4,
RobustConv -- with a concat slice written by a grouped conv, an upsample read from one, and a
two-level IDetect head. Dense convs keep cin in {32, 64, 128k} (the MFMA tiles' rule).
tests/golden/make_golden_grouped.py records the reference's outputs for it (g6_grouped.npz / .json).

RobustConv's layer scale: the reference initialises gamma to 1e-6 and the synthetic weights keep
parameters they do not know, which would scale the block's signal away and hide an error in it;
the config passes layer_scale_init_value = 0.75 (the constructor's last argument) instead."""
NC = 3
ANCHORS2 = [[10, 13, 16, 30, 33, 23], [30, 61, 62, 45, 59, 119]]  # two levels, 3 anchors each
SHAPE = (2, 3, 64, 64)
IMG_SEED, W_SEED = 600, 23
STRIDES = [4.0, 8.0]
OUT_LAYERS = [17, 13]  # strides 4, 8
N_GCONV = 7            # layers 2, 4, 6 (cv2), 8 (m.0.cv2), 11 (cv2), 12 (conv_dw), 13

_BACKBONE = [
    [-1, 1, 'Conv', [32, 3, 1]],                 # 0   32 @ 64
    [-1, 1, 'Conv', [64, 3, 2]],                 # 1   64 @ 32
    [-1, 1, 'dw_conv', [64, 3, 2]],              # 2   64 @ 16  depthwise k3 s2
    [-1, 1, 'Conv', [64, 1, 1]],                 # 3   64 @ 16
    [-2, 1, 'dw_conv', [64, 5, 1]],              # 4   64 @ 16  depthwise k5 s1, into a concat slice
    [[-1, -2], 1, 'Concat', [1]],                # 5  128 @ 16
    [-1, 1, 'ResX', [128]],                      # 6  128 @ 16  g 32: cin_g 2, shortcut added
    [-1, 1, 'Conv', [128, 3, 2]],                # 7  128 @ 8
    [-1, 1, 'ResXCSPC', [256]],                  # 8  256 @ 8   g 32 on 128: cin_g 4
    [-1, 1, 'ResCSPA', [128]],                   # 9  128 @ 8   g 1: dense 3x3 on 32 channels
    [-1, 1, 'Conv', [64, 1, 1]],                 # 10  64 @ 8
    [-1, 1, 'Bottleneck', [64, True, 4, 1.0]],   # 11  64 @ 8   g 4 on 64: cin_g 16, shortcut added
    [-1, 1, 'RobustConv', [128, 7, 1, 'None', 1, True, 0.75]],  # 12 128 @ 8  depthwise k7 + biased 1x1 * gamma
]
_HEAD = [
    [-1, 1, 'dw_conv', [128, 3, 1]],                  # 13 128 @ 8   read by the upsample and by the head
    [-1, 1, 'nn.Upsample', ['None', 2, 'nearest']],   # 14 128 @ 16  (a grouped producer: the copy kernel)
    [[-1, 6], 1, 'Concat', [1]],                      # 15 256 @ 16
    [-1, 1, 'Conv', [128, 1, 1]],                     # 16 128 @ 16
    [-1, 1, 'Conv', [128, 3, 1]],                     # 17 128 @ 16
]


def _copy(rows):
    return [[list(f) if isinstance(f, list) else f, n, m, list(a)] for f, n, m, a in rows]


def gx_mini():
    return {'depth_multiple': 1.0, 'width_multiple': 1.0, 'backbone': _copy(_BACKBONE),
            'head': _copy(_HEAD) + [[list(OUT_LAYERS), 1, 'IDetect', ['nc', 'anchors']]]}


def single(module, args, c_in=64):
    """One block on its own behind a dense stem (parse / plan tests): stem 3 -> 32, 3x3 s2 -> c_in, block."""
    return {'depth_multiple': 1.0, 'width_multiple': 1.0, 'head': [],
            'backbone': [[-1, 1, 'Conv', [32, 3, 1]], [-1, 1, 'Conv', [c_in, 3, 2]], [-1, 1, module, list(args)]]}


# every new module name with constructor arguments the grouped kernel takes (ResX* on 128 channels)
SINGLES = {
    'dw_conv': ('dw_conv', [64, 3, 1], 64),
    'Res': ('Res', [64], 64),
    'ResX': ('ResX', [128], 128),
    'ResCSPA': ('ResCSPA', [64], 64), 'ResCSPB': ('ResCSPB', [64], 64), 'ResCSPC': ('ResCSPC', [64], 64),
    'ResXCSPA': ('ResXCSPA', [256], 128), 'ResXCSPB': ('ResXCSPB', [128], 128), 'ResXCSPC': ('ResXCSPC', [256], 128),
    'RobustConv': ('RobustConv', [64, 7, 1], 64),
}
