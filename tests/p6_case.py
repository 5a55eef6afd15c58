"""The shared P6 test network ("p6-mini"): ReOrg stem, DownC stages down to stride 64, SPPCSPC, a
top-down head and four output maps (strides 8, 16, 32, 64), ending in IDetect or IAuxDetect.
Widths stay within 32..256 so every conv meets the MFMA tiles' cin rules (32, 64, 128k).
tests/golden/make_golden_p6.py records the reference's outputs for it (g5_p6.npz / g5_p6.json)."""
NC = 3
ANCHORS4 = [[19, 27, 44, 40, 38, 94], [96, 68, 86, 152, 180, 137], [140, 301, 303, 264, 238, 542],
            [436, 615, 739, 380, 925, 792]]  # four levels, 12 pairs (the yolov7-w6 anchors)
SHAPE = (2, 3, 128, 128)
IMG_SEED, W_SEED = 500, 21
STRIDES = [8.0, 16.0, 32.0, 64.0]
OUT_LAYERS = [31, 26, 21, 16]  # strides 8, 16, 32, 64
AUX_LAYERS = [10, 12, 14, 15]  # same map sizes as the main inputs (nets/iaux_detect.py:37-38)

_BACKBONE = [
    [-1, 1, 'ReOrg', []],                 # 0   12 @ 64
    [-1, 1, 'Conv', [64, 3, 1]],          # 1   64 @ 64
    [-1, 1, 'Conv', [128, 3, 2]],         # 2  128 @ 32
    [-1, 1, 'Conv', [64, 1, 1]],          # 3  ELAN-style block
    [-2, 1, 'Conv', [64, 1, 1]],          # 4
    [-1, 1, 'Conv', [64, 3, 1]],          # 5
    [-1, 1, 'Conv', [64, 3, 1]],          # 6
    [[-1, -2, -3, -4], 1, 'Concat', [1]],  # 7  256
    [-1, 1, 'Conv', [128, 1, 1]],         # 8  128 @ 32
    [-1, 1, 'DownC', [128]],              # 9  128 @ 16  (stride 8)
    [-1, 1, 'Conv', [128, 3, 1]],         # 10
    [-1, 1, 'DownC', [256]],              # 11 256 @ 8   (stride 16)
    [-1, 1, 'Conv', [256, 1, 1]],         # 12
    [-1, 1, 'DownC', [256]],              # 13 256 @ 4   (stride 32)
    [-1, 1, 'Conv', [256, 1, 1]],         # 14
    [-1, 1, 'DownC', [256]],              # 15 256 @ 2   (stride 64)
    [-1, 1, 'SPPCSPC', [128]],            # 16 128 @ 2
]
_HEAD = [
    [-1, 1, 'Conv', [128, 1, 1]],                     # 17
    [-1, 1, 'nn.Upsample', ['None', 2, 'nearest']],   # 18 @ 4
    [14, 1, 'Conv', [128, 1, 1]],                     # 19
    [[-1, -2], 1, 'Concat', [1]],                     # 20 256
    [-1, 1, 'Conv', [128, 3, 1]],                     # 21 128 @ 4
    [-1, 1, 'Conv', [128, 1, 1]],                     # 22
    [-1, 1, 'nn.Upsample', ['None', 2, 'nearest']],   # 23 @ 8
    [12, 1, 'Conv', [128, 1, 1]],                     # 24
    [[-1, -2], 1, 'Concat', [1]],                     # 25 256
    [-1, 1, 'Conv', [128, 3, 1]],                     # 26 128 @ 8
    [-1, 1, 'Conv', [64, 1, 1]],                      # 27
    [-1, 1, 'nn.Upsample', ['None', 2, 'nearest']],   # 28 @ 16
    [10, 1, 'Conv', [64, 1, 1]],                      # 29
    [[-1, -2], 1, 'Concat', [1]],                     # 30 128
    [-1, 1, 'Conv', [64, 3, 1]],                      # 31  64 @ 16
]


def _copy(rows):
    return [[list(f) if isinstance(f, list) else f, n, m, list(a)] for f, n, m, a in rows]


def p6_mini(head='IDetect'):
    """The config dict; head 'IDetect' (four inputs) or 'IAuxDetect' (four main + four aux inputs)."""
    src = OUT_LAYERS + (AUX_LAYERS if head == 'IAuxDetect' else [])
    return {'depth_multiple': 1.0, 'width_multiple': 1.0, 'backbone': _copy(_BACKBONE),
            'head': _copy(_HEAD) + [[list(src), 1, head, ['nc', 'anchors']]]}


# A DownC block on its own (k2 pool): ReOrg stem, one stride-2 conv, then DownC as the model output.
DOWNC_SHAPE = (2, 3, 64, 64)
DOWNC_IMG_SEED, DOWNC_W_SEED = 501, 22


def downc_block():
    return {'depth_multiple': 1.0, 'width_multiple': 1.0, 'head': [],
            'backbone': [[-1, 1, 'ReOrg', []], [-1, 1, 'Conv', [64, 3, 1]], [-1, 1, 'Conv', [128, 3, 2]],
                         [-1, 1, 'DownC', [128]]]}


VARIANTS = {'idetect': 'IDetect', 'iauxdetect': 'IAuxDetect'}
