"""ycx_ibin_decode on its own: seeded fp32 heads through the kernel against a torch CPU restatement of the
reference's eval branch (nets/ibin.py:55-72 with losses/sigmoid_bin.py:49-63), written here.

Shapes, the smallest that can go wrong: 5 x 7 (fewer cells than a block, odd sides), 9 x 8 (72 cells: one
past a 64-cell block), 20 x 20 (several blocks and a tail); na in {1, 3}; nc in {1, 3, 80}, i.e. raw
widths no = 48 (even: padded LDS rows), 50 (even) and 127 (odd, 64 cells fill the 64 KB), always at
row_off > 0 inside a larger rows_total.

Exact: xview is the permuted input bit for bit; z and xview lie in sentinel frames that must stay
untouched; the columns that IDetect's decode computes the same way (x, y, objectness, classes) equal
ycx_idetect_decode's bit for bit on the same logits; crafted rows (equal bins, the maximum at 0 / 10 / 20,
two equal maxima, both clamps through saturated +-40 logits, a NaN outside the bins) are exact.

Tolerance of the random heads, column-wise max |gpu - ref| / max |ref|: IDETECT_REL_ERR is what the
existing ycx_idetect_decode (the same ycx_sigmoid) measures against oracle.ref_post.idetect_eval on these
shapes with N(0, 2) logits (tests/probes/ibin_bench.py tol, recorded in profiles/ibin/README.md); every
column is allowed 4x that: the regression term adds two multiplies, and the anchor scales it.

The arg-max is discontinuous: a row's w (or h) is left out of the comparison only if torch's two largest
sigmoid'd bin scores of that group are equal or at most 2 fp32 ulp apart, and at most 1 % of the rows may
be (asserted; N(0, 2) logits are far from saturation)."""
import ctypes

import pytest
import torch

from helpers import SENTINEL_F32, fetch_out, guarded_out
from ycx import _lib as L

pytestmark = pytest.mark.gpu

BINS = 21
GROUP = BINS + 1
STEP = 4.0 / BINS  # SigmoidBin.step for min 0, max 4 (a Python float, as in the reference)
# max |gpu - ref| / max |ref| of ycx_idetect_decode vs oracle.ref_post.idetect_eval over SHAPES x na x nc
# below with the same N(0, 2) logits (measured on an MI355X: 2.3286e-07 at 9 x 8, na 3, nc 80, in the w / h
# columns; profiles/ibin/README.md has every case). ycx_ibin_decode's own largest column figure was 1.24e-07.
IDETECT_REL_ERR = 2.33e-7
TOL = 4 * IDETECT_REL_ERR  # 9.3e-07
MAX_SKIPPED = 0.01
SHAPES = [(5, 7), (9, 8), (20, 20)]
ANCHORS = [10.0, 13.0, 16.0, 30.0, 33.0, 23.0]
ROW_OFF, ROW_TAIL = 5, 3
N = 2


def bin_centres():
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return torch.range(STEP / 2, 4.0 - STEP / 2 + 0.0001, STEP).float()


def sigmoid_bin_forward(pred, bins):
    """losses/sigmoid_bin.py:49-63 on already sigmoid'd scores, use_fw_regression on."""
    pred_reg = (pred[..., 0] * 2.0 - 2.0 / 2.0) * STEP
    _, bin_idx = torch.max(pred[..., 1:1 + BINS], dim=-1)
    return (pred_reg + bins[bin_idx]).clamp(min=0.0, max=4.0)


def ibin_level_ref(head, anchors, na, stride, w_bins, h_bins):
    """One level of nets/ibin.py:48-72 on a raw fp32 NCHW map: (z (bs, na*ny*nx, nc + 5), x (bs, na, ny, nx,
    no), the sigmoid'd scores (bs, na, ny, nx, no))."""
    bs, ch, ny, nx = head.shape
    x = head.view(bs, na, ch // na, ny, nx).permute(0, 1, 3, 4, 2).contiguous()
    z, p = ibin_rows_ref(x, anchors, stride, w_bins, h_bins)
    return z, x, p


def ibin_rows_ref(x, anchors, stride, w_bins, h_bins):
    """nets/ibin.py:51-72 on the re-laid map x (bs, na, ny, nx, no): (z, the sigmoid'd scores)."""
    bs, na, ny, nx, _ = x.shape
    yv, xv = torch.meshgrid([torch.arange(ny), torch.arange(nx)], indexing='ij')
    grid = torch.stack((xv, yv), 2).view((1, 1, ny, nx, 2)).float()
    anchor_grid = torch.tensor(anchors[:2 * na]).float().view(1, na, 1, 1, 2)
    y = x.sigmoid()
    p = y.clone()
    y[..., 0:2] = (y[..., 0:2] * 2. - 0.5 + grid) * torch.tensor(stride, dtype=torch.float32)
    pw = sigmoid_bin_forward(y[..., 2:24], w_bins) * anchor_grid[..., 0]
    ph = sigmoid_bin_forward(y[..., 24:46], h_bins) * anchor_grid[..., 1]
    y[..., 2] = pw
    y[..., 3] = ph
    y = torch.cat((y[..., 0:4], y[..., 46:]), dim=-1)
    return y.view(bs, -1, y.shape[-1]), p


def near_tie(p):
    """(rows, 2) mask over (w, h): torch's two largest sigmoid'd bin scores are equal or <= 2 fp32 ulp apart."""
    out = []
    for lo in (3, 3 + GROUP):
        top = p[..., lo:lo + BINS].reshape(-1, BINS).topk(2, -1).values.contiguous()
        bits = top.view(torch.int32).long()  # positive floats: the bit patterns count representable values
        out.append((bits[:, 0] - bits[:, 1]) <= 2)
    return torch.stack(out, 1)


def desc(n, h, w, na, no, rows_total, row_off, anchors=ANCHORS):
    d = L.DecodeDesc()
    d.n, d.h, d.w, d.na, d.no, d.rows_total, d.row_off = n, h, w, na, no, rows_total, row_off
    for a in range(2 * na):
        d.anchors_scaled[a] = anchors[a]
    return d


def run_ibin(device, head, na, stride, w_bins, h_bins, row_off=ROW_OFF, row_tail=ROW_TAIL):
    """The kernel on ``head`` (CPU fp32 NCHW): returns the whole z buffer [n][row_off + rows + tail][nz] and
    xview, both fetched from sentinel-framed allocations whose guards are checked."""
    n, ch, h, w = head.shape
    no = ch // na
    nz = no - 2 * GROUP + 2
    rows = na * h * w
    total = row_off + rows + row_tail
    z = guarded_out(torch.full((n, total, nz), SENTINEL_F32), device)
    xv = guarded_out(torch.full((n, na, h, w, no), SENTINEL_F32), device)
    hd = head.to(device).contiguous()
    d = desc(n, h, w, na, no, total, row_off)
    wb, hb = ((ctypes.c_float * BINS)(*b.tolist()) for b in (w_bins, h_bins))
    L.check(L.lib.ycx_ibin_decode(ctypes.byref(d), ctypes.c_float(stride), BINS, wb, hb, hd.data_ptr(), z.data_ptr(),
                                  xv.data_ptr(), L.stream_handle(device)), "ycx_ibin_decode")
    torch.cuda.synchronize()
    return fetch_out(z, SENTINEL_F32, what='z'), fetch_out(xv, SENTINEL_F32, what='xview')


def run_idetect(device, head, na, stride):
    n, ch, h, w = head.shape
    no = ch // na
    z = torch.empty((n, na * h * w, no), dtype=torch.float32, device=device)
    xv = torch.empty((n, na, h, w, no), dtype=torch.float32, device=device)
    hd = head.to(device).contiguous()
    d = desc(n, h, w, na, no, na * h * w, 0)
    L.check(L.lib.ycx_idetect_decode(ctypes.byref(d), ctypes.c_float(stride), hd.data_ptr(), z.data_ptr(),
                                     xv.data_ptr(), L.stream_handle(device)), "ycx_idetect_decode")
    torch.cuda.synchronize()
    return z.cpu()


def random_head(h, w, na, nc, seed):
    no = nc + 3 + 2 * GROUP
    g = torch.Generator().manual_seed(seed)
    return torch.randn((N, na * no, h, w), generator=g) * 2.0  # N(0, 2): far from saturation


def col_err(got, ref):
    """max |got - ref| / max |ref| per column of (rows, cols) tensors, in float64."""
    got, ref = got.double(), ref.double()
    return (got - ref).abs().amax(0) / ref.abs().amax(0).clamp_min(1e-30)


def compare_z(z_gpu, z_ref, p, what):
    """Column-wise comparison of decoded rows under TOL with the near-tie skip rule; returns the figures."""
    nz = z_ref.shape[-1]
    got, ref = z_gpu.reshape(-1, nz), z_ref.reshape(-1, nz)
    skip = near_tie(p)
    share = float(skip.any(1).double().mean())
    errs = col_err(got, ref)
    for j in (0, 1):  # w, h: without the skipped rows
        keep = ~skip[:, j]
        errs[2 + j] = col_err(got[keep, 2 + j:3 + j], ref[keep, 2 + j:3 + j])[0]
    fig = dict(xy=float(errs[:2].max()), wh=float(errs[2:4].max()), conf=float(errs[4:].max()), skipped=share,
               flips=int((got[:, 2:4] != ref[:, 2:4]).sum()))
    print(f"\n{what}: {fig}")
    assert share <= MAX_SKIPPED, fig
    assert float(errs.max()) < TOL, fig
    return fig


@pytest.mark.parametrize('nc', [1, 3, 80])
@pytest.mark.parametrize('na', [1, 3])
@pytest.mark.parametrize('h, w', SHAPES)
def test_random_heads(device, h, w, na, nc):
    no = nc + 3 + 2 * GROUP
    head = random_head(h, w, na, nc, seed=1000 + 100 * h + 10 * na + nc)
    bins = bin_centres()
    stride = 8.0
    z_ref, x_ref, p = ibin_level_ref(head, ANCHORS, na, stride, bins, bins)
    z_all, xv = run_ibin(device, head, na, stride, bins, bins)
    rows = na * h * w
    # xview: the permuted input, bit for bit
    assert torch.equal(xv.view(torch.int32), x_ref.view(torch.int32))
    # the frame: rows before row_off and after the level stay the sentinel
    assert bool((z_all[:, :ROW_OFF] == SENTINEL_F32).all()) and bool((z_all[:, ROW_OFF + rows:] == SENTINEL_F32).all())
    z = z_all[:, ROW_OFF:ROW_OFF + rows]
    assert tuple(z.shape) == tuple(z_ref.shape) == (N, rows, nc + 5) and not bool((z == SENTINEL_F32).any())
    compare_z(z, z_ref, p, f"ibin decode {h}x{w} na={na} nc={nc} (no={no})")
    # x, y, objectness and classes are IDetect's expressions on the same logits and the same ycx_sigmoid
    x5 = head.view(N, na, no, h, w)
    same = torch.cat([x5[:, :, 0:3], x5[:, :, 2 + GROUP:3 + GROUP], x5[:, :, 2 + 2 * GROUP:]], 2)
    zi = run_idetect(device, same.reshape(N, na * (nc + 5), h, w).contiguous(), na, stride)
    cols = [0, 1] + list(range(4, nc + 5))
    assert torch.equal(z[..., cols].contiguous().view(torch.int32), zi[..., cols].contiguous().view(torch.int32))


def test_distinct_bin_tables_and_anchors(device):
    """w reads w_bins and the anchor's width, h reads h_bins and its height (the two tables differ here)."""
    head = random_head(9, 8, 3, 3, seed=77)
    w_bins = bin_centres()
    h_bins = torch.flip(w_bins, [0]) * 0.5
    z_ref, _, p = ibin_level_ref(head, ANCHORS, 3, 16.0, w_bins, h_bins)
    z_all, _ = run_ibin(device, head, 3, 16.0, w_bins, h_bins)
    compare_z(z_all[:, ROW_OFF:ROW_OFF + 3 * 72], z_ref, p, "ibin decode, distinct tables")


def crafted_head():
    """(1, no, 5, 7) with na 1, nc 3: cell c of the flattened map holds case c; the rest is zero logits."""
    no = 3 + 3 + 2 * GROUP
    x = torch.zeros((1, 1, 35, no))
    wb, hb = slice(3, 3 + BINS), slice(3 + GROUP, 3 + GROUP + BINS)
    want = {}  # cell -> (w bin index, h bin index, w regression sign, h regression sign)
    want[0] = (0, 0, 0, 0)                                   # all bin logits equal: index 0
    for c, k in ((1, 0), (2, 10), (3, 20)):                  # the maximum at 0, 10, 20
        x[0, 0, c, wb] = -5.0
        x[0, 0, c, hb] = -5.0
        x[0, 0, c, 3 + k] = 3.0
        x[0, 0, c, 3 + GROUP + (20 - k)] = 3.0
        want[c] = (k, 20 - k, 0, 0)
    x[0, 0, 4, wb] = -5.0                                    # two equal maxima: the lower index
    x[0, 0, 4, [3 + 4, 3 + 15]] = 3.0
    x[0, 0, 4, hb] = 1.0
    x[0, 0, 4, [3 + GROUP + 20, 3 + GROUP + 19]] = 2.0
    want[4] = (4, 19, 0, 0)
    x[0, 0, 5, wb] = -40.0                                   # saturated: the upper clamp (bin 20 + step > 4)
    x[0, 0, 5, 3 + 20] = 40.0
    x[0, 0, 5, 2] = 40.0
    x[0, 0, 5, hb] = -40.0                                   # ... and the lower (bin 0 - step < 0)
    x[0, 0, 5, 3 + GROUP] = 40.0
    x[0, 0, 5, 2 + GROUP] = -40.0
    want[5] = (20, 0, 1, -1)
    x[0, 0, 6, wb] = 40.0                                    # every score saturates to 1.0: a tie, index 0
    x[0, 0, 6, 2] = -40.0
    x[0, 0, 6, hb] = -40.0                                   # every score is the same tiny value: index 0
    x[0, 0, 6, 2 + GROUP] = 40.0
    want[6] = (0, 0, -1, 1)
    return x.view(1, 1, 5, 7, no).permute(0, 1, 4, 2, 3).reshape(1, no, 5, 7).contiguous(), want


def test_crafted_rows_are_exact(device):
    head, want = crafted_head()
    bins = bin_centres()
    aw, ah = torch.tensor(ANCHORS[0]), torch.tensor(ANCHORS[1])
    z_ref, _, _ = ibin_level_ref(head, ANCHORS, 1, 8.0, bins, bins)
    z_all, _ = run_ibin(device, head, 1, 8.0, bins, bins)
    z = z_all[0, ROW_OFF:ROW_OFF + 35]
    step = torch.tensor(STEP, dtype=torch.float32)
    for c, (kw, kh, sw, sh) in want.items():
        # sigmoid(0) = 0.5 and sigmoid(+-40) = 1 / 0 (to within what * 2 - 1 rounds away) are exact
        exp_w = (sw * step + bins[kw]).clamp(0.0, 4.0) * aw
        exp_h = (sh * step + bins[kh]).clamp(0.0, 4.0) * ah
        assert float(z_ref[0, c, 2]) == float(exp_w) and float(z_ref[0, c, 3]) == float(exp_h), c  # the restatement
        assert float(z[c, 2]) == float(exp_w) and float(z[c, 3]) == float(exp_h), (c, z[c, :4], exp_w, exp_h)
    assert float(z[5, 2]) == 4.0 * ANCHORS[0] and float(z[5, 3]) == 0.0  # both clamps were hit
    assert float(z[6, 2]) == 0.0 and float(z[6, 3]) == float((step + bins[0]) * ah)
    # every untouched cell is case 0
    assert torch.equal(z[7:, 2:4], z[0:1, 2:4].expand(28, 2))
    assert torch.equal(z[:, 2:4], z_ref[0, :, 2:4])


def test_nan_outside_the_bins_stays_in_its_column(device):
    """A NaN logit in x, in a class, or in the w regression slot changes that one z column of that one row."""
    head = random_head(5, 7, 1, 3, seed=31)[:1]
    no = head.shape[1]
    bins = bin_centres()
    clean, _ = run_ibin(device, head, 1, 8.0, bins, bins)
    dirty_head = head.clone()
    cells = {(0, 3): 0, (47, 20): 5, (2, 9): 2}  # (raw column, cell) -> z column
    for (col, cell) in cells:
        dirty_head[0, col, cell // 7, cell % 7] = float('nan')
    dirty, xv = run_ibin(device, dirty_head, 1, 8.0, bins, bins)
    assert int(xv.isnan().sum()) == 3
    z0, z1 = clean[0, ROW_OFF:ROW_OFF + 35], dirty[0, ROW_OFF:ROW_OFF + 35]
    hit = torch.zeros_like(z0, dtype=torch.bool)
    for (col, cell), zc in cells.items():
        hit[cell, zc] = True
    assert bool(z1[hit].isnan().all()) and int(z1.isnan().sum()) == 3
    assert torch.equal(z1[~hit].view(torch.int32), z0[~hit].view(torch.int32))
    assert no == 50
