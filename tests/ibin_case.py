"""The shared IBin test network ("ibin-mini"): a four-Conv backbone down to two levels (strides 8 and 16
of a 64 x 64 image) and a two-level IBin head with three anchors per level. nc = 3 makes the head's raw
width no = nc + 3 + 2 * (21 + 1) = 50, an even number (ycx_ibin_decode pads its LDS rows then), and the
head convs 150 channels wide (cout_pad 256 / 192). Dense convs keep cin in {32, 64, 128k} (the MFMA tiles'
rule). tests/golden/make_golden_ibin.py records the reference's outputs for it (g12_ibin.npz / .json)."""
NC = 3
BIN_COUNT = 21
NO = NC + 3 + 2 * (BIN_COUNT + 1)  # 50
NZ = NC + 5
ANCHORS2 = [[10, 13, 16, 30, 33, 23], [30, 61, 62, 45, 59, 119]]  # two levels, 3 anchors each
NA = 3
SHAPE = (2, 3, 64, 64)
# seeds picked on the reference's own output: 2 of its 480 rows have top-two bin logits within the f32 bar
# (the generator asserts <= 1 %); most neighbouring seeds give 3 to 7
IMG_SEED, W_SEED = 1200, 39
STRIDES = [8.0, 16.0]
OUT_LAYERS = [2, 3]
ROWS = [NA * 8 * 8, NA * 4 * 4]
NC_WIDE = 80  # the shipped class count: no = 127, head convs 381 wide (cout_pad 384)

_BACKBONE = [
    [-1, 1, 'Conv', [32, 3, 2]],            # 0   32 @ 32
    [-1, 1, 'Conv', [64, 3, 2]],            # 1   64 @ 16
    [-1, 1, 'Conv', [128, 3, 2]],           # 2  128 @ 8    stride 8
    [-1, 1, 'Conv', [128, 3, 2]],           # 3  128 @ 4    stride 16
]


def _copy(rows):
    return [[list(f) if isinstance(f, list) else f, n, m, list(a)] for f, n, m, a in rows]


def ibin_mini(head='IBin'):
    """The config dict, in the reference's YAML spelling [[...], 1, IBin, [nc, anchors]] (the builder
    appends the input channel list as the third argument, so a YAML cannot name a bin_count)."""
    return {'depth_multiple': 1.0, 'width_multiple': 1.0, 'backbone': _copy(_BACKBONE),
            'head': [[list(OUT_LAYERS), 1, head, ['nc', 'anchors']]]}
