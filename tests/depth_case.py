"""The shared space/depth test network ("sd-mini"): a Focus stem on the image (ReOrg's gather folded into
its 3x3 conv: ``stem_reorg``), Contract(2) feeding a Conv, Expand(2) of a 128-channel map written into a
Concat slice (the aliasing case), a Focus that reads an activation (a focus-mode 'depth' node, then its
1x1 conv), and a two-level IDetect head. ``sd_mini('conv')`` is the same network behind a plain Conv stem.
Dense convs keep cin in {32, 64, 128k} (the MFMA tiles' rule) and every moved channel run is a multiple of
8. tests/golden/make_golden_depth.py records the reference's outputs for it (g11_depth.npz / .json)."""
NC = 2
ANCHORS2 = [[10, 13, 16, 30, 33, 23], [30, 61, 62, 45, 59, 119]]  # two levels, 3 anchors each
SHAPE = (2, 3, 64, 64)
IMG_SEED, W_SEED = 1100, 31
STRIDES = [4.0, 8.0]
OUT_LAYERS = [8, 9]  # strides 4, 8
# 'depth' nodes: layer 2 (contract2), layer 5 (expand2), layer 7 (focus2)
N_DEPTH = 3
DEPTH_NAMES = ['contract2', 'expand2', 'focus2']
SINGLE_SHAPE = (1, 3, 48, 48)  # the block sees a 24 x 24 map: divisible by every gain

_STEMS = {'focus': [-1, 1, 'Focus', [32, 3]],      # 0   32 @ 32  Conv(12, 32, 3, 1) over the four pixel phases
          'conv': [-1, 1, 'Conv', [32, 3, 2]]}     # 0   32 @ 32
_BACKBONE = [
    [-1, 1, 'Conv', [64, 3, 2]],            # 1   64 @ 16
    [-1, 1, 'Contract', [2]],               # 2  256 @ 8
    [-1, 1, 'Conv', [128, 1, 1]],           # 3  128 @ 8
    [1, 1, 'Conv', [32, 1, 1]],             # 4   32 @ 16
]
_HEAD = [
    [3, 1, 'Expand', [2]],                  # 5   32 @ 16  written into layer 6's concat slice
    [[-1, 4], 1, 'Concat', [1]],            # 6   64 @ 16
    [-1, 1, 'Focus', [64, 1]],              # 7   64 @ 8   reads an activation: depth (focus) + Conv(256, 64, 1, 1)
    [6, 1, 'Conv', [128, 3, 1]],            # 8  128 @ 16
    [7, 1, 'Conv', [128, 3, 1]],            # 9  128 @ 8
]


def _copy(rows):
    return [[list(f) if isinstance(f, list) else f, n, m, list(a)] for f, n, m, a in rows]


def sd_mini(stem='focus'):
    return {'depth_multiple': 1.0, 'width_multiple': 1.0, 'backbone': _copy([_STEMS[stem]] + _BACKBONE),
            'head': _copy(_HEAD) + [[list(OUT_LAYERS), 1, 'IDetect', ['nc', 'anchors']]]}


def single(module, args, c_in=64):
    """One block on its own behind a dense stem (parse / plan tests): stem 3 -> 32, 3x3 s2 -> c_in, block."""
    return {'depth_multiple': 1.0, 'width_multiple': 1.0, 'head': [],
            'backbone': [[-1, 1, 'Conv', [32, 3, 1]], [-1, 1, 'Conv', [c_in, 3, 2]], [-1, 1, module, list(args)]]}


def on_input(module, args):
    """The same module as layer 0, reading the image."""
    return {'depth_multiple': 1.0, 'width_multiple': 1.0, 'head': [], 'backbone': [[-1, 1, module, list(args)]]}


# every new module name in the reference's YAML spelling: (module, args, c_in, the depth op's name)
SINGLES = {
    'Focus': ('Focus', [64, 3], 64, 'focus2'),
    'Focus_k1': ('Focus', [64, 1], 32, 'focus2'),
    'Focus_g8': ('Focus', [64, 3, 1, 'None', 8], 16, 'focus2'),   # a grouped conv behind the move
    'Contract': ('Contract', [2], 64, 'contract2'),
    'Contract3': ('Contract', [3], 64, 'contract3'),
    'Contract4': ('Contract', [4], 32, 'contract4'),
    'Expand': ('Expand', [2], 64, 'expand2'),
    'Expand3': ('Expand', [3], 72, 'expand3'),
    'Expand4': ('Expand', [4], 128, 'expand4'),
}
