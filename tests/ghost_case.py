"""The shared Ghost-family test network ("gh-mini"): GhostConv with k1 / s1 and k3 / s2, Ghost with
stride 1 (the block input is the shortcut) and stride 2 (depthwise + 1x1 shortcut), GhostCSPA / B / C,
GhostSPPCSPC, a Ghost output written into an outer Concat slice, a GhostConv output read by an
upsample, and a two-level IDetect head. Every Ghost-family module sits behind the dense stem, never
on the image. Dense convs keep cin in {32, 64, 128k} (the MFMA tiles' rule), so a Ghost block has
c2 in {64, 128, 256k}, which also keeps every GhostConv's hidden width a multiple of 8.
tests/golden/make_golden_ghost.py records the reference's outputs for it (g9_ghost.npz / .json)."""
NC = 3
ANCHORS2 = [[10, 13, 16, 30, 33, 23], [30, 61, 62, 45, 59, 119]]  # two levels, 3 anchors each
SHAPE = (2, 3, 64, 64)
IMG_SEED, W_SEED = 900, 29
STRIDES = [4.0, 8.0]
OUT_LAYERS = [15, 9]  # strides 4, 8
# 'ghost' nodes per layer: 2: 1, 3: 1, 4: 2, 5: 2, 6: 2, 7: 2, 8: 2, 9: 7, 10: 1, 12: 2
N_GHOST = 22
N_GHOST_RES = 6  # one per Ghost block: layers 4, 5, 6, 7, 8, 12
N_GCONV = 2      # layer 5: the depthwise 3x3 / s2 of its conv branch and of its shortcut

_BACKBONE = [
    [-1, 1, 'Conv', [32, 3, 1]],            # 0   32 @ 64
    [-1, 1, 'Conv', [64, 3, 2]],            # 1   64 @ 32
    [-1, 1, 'GhostConv', [64, 1, 1]],       # 2   64 @ 32  k1 s1, hidden 32
    [-1, 1, 'GhostConv', [128, 3, 2]],      # 3  128 @ 16  k3 s2, hidden 64
    [-1, 1, 'Ghost', [128, 3, 1]],          # 4  128 @ 16  s1: layer 3's map is the shortcut
    [-1, 1, 'Ghost', [256, 3, 2]],          # 5  256 @ 8   s2: dw 3x3 / s2 between the GhostConvs, dw + 1x1 shortcut
    [-1, 1, 'GhostCSPA', [128]],            # 6  128 @ 8   Ghost(64, 64): hidden widths 16 and 32
    [-1, 1, 'GhostCSPB', [128]],            # 7  128 @ 8   Ghost(128, 128)
    [-1, 1, 'GhostCSPC', [128]],            # 8  128 @ 8   Ghost(64, 64)
    [-1, 1, 'GhostSPPCSPC', [128]],         # 9  128 @ 8   seven GhostConvs around the pool cascade
]
_HEAD = [
    [-1, 1, 'GhostConv', [128, 1, 1]],                # 10 128 @ 8   read by the upsample (the copy kernel)
    [-1, 1, 'nn.Upsample', ['None', 2, 'nearest']],   # 11 128 @ 16
    [4, 1, 'Ghost', [128, 3, 1]],                     # 12 128 @ 16  written into layer 13's concat slice
    [[-1, 11], 1, 'Concat', [1]],                     # 13 256 @ 16
    [-1, 1, 'Conv', [128, 1, 1]],                     # 14 128 @ 16
    [-1, 1, 'Conv', [128, 3, 1]],                     # 15 128 @ 16
]


def _copy(rows):
    return [[list(f) if isinstance(f, list) else f, n, m, list(a)] for f, n, m, a in rows]


def gh_mini():
    return {'depth_multiple': 1.0, 'width_multiple': 1.0, 'backbone': _copy(_BACKBONE),
            'head': _copy(_HEAD) + [[list(OUT_LAYERS), 1, 'IDetect', ['nc', 'anchors']]]}


def single(module, args, c_in=64):
    """One block on its own behind a dense stem (parse / plan tests): stem 3 -> 32, 3x3 s2 -> c_in, block."""
    return {'depth_multiple': 1.0, 'width_multiple': 1.0, 'head': [],
            'backbone': [[-1, 1, 'Conv', [32, 3, 1]], [-1, 1, 'Conv', [c_in, 3, 2]], [-1, 1, module, list(args)]]}


def on_input(module, args):
    """The same module as layer 0, reading the image: out of scope at parse time."""
    return {'depth_multiple': 1.0, 'width_multiple': 1.0, 'head': [], 'backbone': [[-1, 1, module, list(args)]]}


# every new module name, with constructor arguments that keep dense cin in {32, 64, 128k}
SINGLES = {
    'GhostConv': ('GhostConv', [64, 1, 1], 64),
    'GhostConv_k3s2': ('GhostConv', [128, 3, 2], 64),
    'Ghost': ('Ghost', [64, 3, 1], 64),
    'Ghost_s2': ('Ghost', [128, 3, 2], 64),
    'GhostCSPA': ('GhostCSPA', [128], 64), 'GhostCSPB': ('GhostCSPB', [64], 64), 'GhostCSPC': ('GhostCSPC', [128], 64),
    'GhostSPPCSPC': ('GhostSPPCSPC', [64], 64),
}
