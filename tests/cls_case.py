"""The shared Classify and Rep-block test networks.

"cls-mini": four Convs down to a 4 x 4 x 64 map of a 64 x 64 image, then Classify [64, 10, 3]: k = 3, so
the conv's weight is [10][64][3][3] and only its centre tap meets the pooled 1 x 1 map.

"rep-mini": RepBottleneck, RepRes, RepResX (g 16 on 64 hidden channels: cin_g 4), RepResCSPA (dense RepConvs)
and RepResXCSPC (g 32 on 64 hidden channels: cin_g 2) behind a dense stem, then a 1x1 Conv that keeps the
recorded output small. Dense convs keep cin in {32, 64, 128k} (the MFMA tiles' rule).

tests/golden/make_golden_cls.py records the reference's outputs for both (g13_cls.npz / .json)."""
NC = 3
ANCHORS2 = [[10, 13, 16, 30, 33, 23], [30, 61, 62, 45, 59, 119]]  # unused by either net; Model wants them
SHAPE = (2, 3, 64, 64)
IMG_SEED, W_SEED = 1300, 41
CLS_C1, CLS_C2, CLS_K = 64, 10, 3

_CLS = [
    [-1, 1, 'Conv', [32, 3, 2]],                  # 0   32 @ 32
    [-1, 1, 'Conv', [64, 3, 2]],                  # 1   64 @ 16
    [-1, 1, 'Conv', [64, 3, 2]],                  # 2   64 @ 8
    [-1, 1, 'Conv', [64, 3, 2]],                  # 3   64 @ 4
]

_REP = [
    [-1, 1, 'Conv', [32, 3, 2]],                  # 0   32 @ 32
    [-1, 1, 'Conv', [64, 3, 2]],                  # 1   64 @ 16
    [-1, 1, 'RepBottleneck', [64]],               # 2   64 @ 16  cv1 64 -> 32, RepConv 32 -> 64, shortcut added
    [-1, 1, 'RepRes', [64]],                      # 3   64 @ 16  RepConv 32 -> 32 with its identity branch
    [-1, 1, 'Conv', [128, 3, 2]],                 # 4  128 @ 8
    [-1, 1, 'RepResX', [128, True, 16]],          # 5  128 @ 8   RepConv 64 -> 64, g 16: cin_g 4
    [-1, 1, 'RepResCSPA', [128]],                 # 6  128 @ 8   m.0 = RepRes(64, 64): RepConv 32 -> 32
    [-1, 1, 'RepResXCSPC', [256]],                # 7  256 @ 8   m.0 = RepResX(128, 128, g 32): RepConv 64 -> 64, cin_g 2
    [-1, 1, 'Conv', [64, 1, 1]],                  # 8   64 @ 8   the recorded output
]
REP_OUT = (2, 64, 8, 8)
# the RepConvs of rep-mini in graph order: (module path under Model.model, groups, node kind)
REP_CONVS = [('2.cv2', 1, 'conv'), ('3.cv2', 1, 'conv'), ('5.cv2', 16, 'gconv'), ('6.m.0.cv2', 1, 'conv'),
             ('7.m.0.cv2', 32, 'gconv')]


def _copy(rows):
    return [[list(f) if isinstance(f, list) else f, n, m, list(a)] for f, n, m, a in rows]


def cls_mini(args=(CLS_C1, CLS_C2, CLS_K), frm=-1):
    """The config dict, in the reference's YAML spelling [-1, 1, Classify, [c1, c2, k, s, p, g]]."""
    return {'depth_multiple': 1.0, 'width_multiple': 1.0, 'backbone': _copy(_CLS),
            'head': [[frm, 1, 'Classify', list(args)]]}


def rep_mini():
    return {'depth_multiple': 1.0, 'width_multiple': 1.0, 'backbone': _copy(_REP), 'head': []}


def single(module, args, c_in=64):
    """One block on its own behind a dense stem (parse / plan tests): stem 3 -> 32, 3x3 s2 -> c_in, block."""
    return {'depth_multiple': 1.0, 'width_multiple': 1.0, 'head': [],
            'backbone': [[-1, 1, 'Conv', [32, 3, 1]], [-1, 1, 'Conv', [c_in, 3, 2]], [-1, 1, module, list(args)]]}


# every Rep name the builder takes, with constructor arguments the kernels take (the X forms on 128 channels)
SINGLES = {
    'RepBottleneck': ('RepBottleneck', [64], 64),
    'RepRes': ('RepRes', [64], 64),
    'RepResX': ('RepResX', [128], 128),
    'RepResCSPA': ('RepResCSPA', [64], 64), 'RepResCSPB': ('RepResCSPB', [64], 64),
    'RepResCSPC': ('RepResCSPC', [64], 64),
    'RepResXCSPA': ('RepResXCSPA', [256], 128), 'RepResXCSPB': ('RepResXCSPB', [128], 128),
    'RepResXCSPC': ('RepResXCSPC', [256], 128),
}
