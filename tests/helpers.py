"""Shared test helpers: build models/state_dicts exactly as the fixtures were made."""
import hashlib

import numpy as np
import torch

from ycx.nets.yolo import Model
from ycx.utils.helper_io import cvt_cfg
from ycx.utils.synth import synthetic_head_logits, synthetic_images, synthetic_state_dict

ANCHORS = [[12, 16, 19, 36, 40, 28], [36, 75, 76, 55, 72, 146], [142, 110, 192, 243, 459, 401]]
MASK = [[6, 7, 8], [3, 4, 5], [0, 1, 2]]


def sd_hash(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def arr_hash(arrs):
    h = hashlib.sha256()
    for a in arrs:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def make_model(cfg, nc, w_seed, precision='bf16'):
    """ycx Model with the fixture's synthetic weights; returns (model, state_dict)."""
    m = Model(cvt_cfg(cfg), ANCHORS, nc, precision=precision).eval()
    sd = synthetic_state_dict(m, seed=w_seed)
    m.load_state_dict(sd)
    return m, sd


def make_model_cfg(cfg, nc, w_seed, precision='bf16'):
    """make_model for a config dict (e.g. a built-in network with its head swapped)."""
    m = Model(cfg, ANCHORS, nc, precision=precision).eval()
    sd = synthetic_state_dict(m, seed=w_seed)
    m.load_state_dict(sd)
    return m, sd


def g1_case(manifest, name, precision='bf16'):
    e = manifest['g1'][name]
    m, sd = make_model(e['cfg'], e['nc'], e['w_seed'], precision)
    x = synthetic_images(*e['shape'], seed=e['img_seed'])
    return m, sd, x, e


def g3_heads(e):
    size, bs = e['size'], e['bs']
    shapes = [(bs, size // 32, size // 32), (bs, size // 16, size // 16), (bs, size // 8, size // 8)]
    return synthetic_head_logits(shapes, e['nc'], seed=e['seed'], obj_shift=e['obj_shift'])


def rel_err(a, b):
    """max |a-b| / max |b| (the tolerance measure used for the 1e-3 parity bound)."""
    a = torch.as_tensor(a, dtype=torch.float64)
    b = torch.as_tensor(b, dtype=torch.float64)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def fused_keep_report(cand, cand_rows, counts, keep, kc, b, heads_b, nc, conf, iou, size, max_det, mask=None):
    """Decompose the fused device path's result for image ``b`` against the
    oracle chain run on the SAME head logits (``heads_b``: CPU fp32 NCHW maps of
    that image, Detect order), so every difference is attributed:

      1. decode: the device's candidate rows and values vs the oracle's
         decode_box + filter (detect.py:29-121) -> ``member_flips`` (rows on one
         side of conf_thres only; each must sit at the threshold) and
         ``box_maxdiff`` (max |xyxy difference| over the common rows);
      2. NMS: the oracle's greedy NMS (torchvision semantics) run on the
         DEVICE's own candidates must give exactly the device's keep rows
         (``nms_exact``; this is the bit-exact-keep-indices claim);
      3. end to end: ``keep_flips`` = |device keep rows ^ oracle keep rows|,
         which can only come from 1. (sigmoid/exp ulps on the device).
    Returns a dict; tests print it and assert on each part."""
    from oracle import ref_post
    A = np.asarray(ANCHORS).reshape(-1, 2)
    dec = torch.cat(ref_post.decode_box([h.unsqueeze(0) if h.dim() == 3 else h for h in heads_b], A, mask or MASK, nc,
                                        (size, size)), 1)
    ref_rows, _ = ref_post.nms_keep_rows(dec.clone(), nc, conf, iou)
    ref_rows = ref_rows[0].numpy()
    # oracle filter on its own decode (xyxy from xywh, score = obj * max cls >= conf)
    d0 = dec[0]
    cls_conf, cls_id = torch.max(d0[:, 5:5 + nc], 1)
    score = d0[:, 4] * cls_conf
    ref_pass = set(torch.nonzero(score >= conf).reshape(-1).tolist())
    # device candidates
    n = int(counts[b])
    rows = np.sort(cand_rows[b, :n].numpy().astype(np.int64))
    c = cand[b, torch.as_tensor(rows)] if n else cand[b, :0]
    cls = c[:, 6].contiguous().view(torch.int32).long()
    row_f = c[:, 7].contiguous().view(torch.int32).long()
    assert torch.equal(row_f, torch.as_tensor(rows)), "ycx_cand.row disagrees with cand_rows"
    dev_pass = set(rows.tolist())
    member = sorted(dev_pass ^ ref_pass)
    # each membership flip must sit at the threshold (|score - conf| a few ulps of conf)
    boundary = [abs(float(score[r]) - conf) for r in member]
    common = sorted(dev_pass & ref_pass)
    box_maxdiff = 0.0
    if common:
        idx = torch.as_tensor(common)
        xywh = d0[idx, :4]
        ref_xyxy = torch.stack([xywh[:, 0] - xywh[:, 2] / 2, xywh[:, 1] - xywh[:, 3] / 2,
                                xywh[:, 0] + xywh[:, 2] / 2, xywh[:, 1] + xywh[:, 3] / 2], 1)
        pos = np.searchsorted(rows, np.asarray(common))
        box_maxdiff = float((c[torch.as_tensor(pos), :4] - ref_xyxy).abs().max())
        cls_same = bool(torch.equal(cls[torch.as_tensor(pos)], cls_id[idx]))
    else:
        cls_same = True
    # oracle NMS on the device's own candidates (class asc, row order within a class)
    own = []
    scores = c[:, 4] * c[:, 5]
    for k in torch.unique(cls).tolist():
        sel = torch.nonzero(cls == k).reshape(-1)
        kept = ref_post.nms(c[sel, :4], scores[sel], iou)
        own.append(torch.as_tensor(rows)[sel[kept]])
    own = torch.cat(own).numpy() if own else np.zeros((0,), np.int64)
    k = int(kc[b])
    got = keep[b, :min(k, max_det)].numpy().astype(np.int64)
    nms_exact = k == len(own) and np.array_equal(got, own[:max_det])
    flipped = set(own.tolist()) ^ set(ref_rows.tolist())
    # explain the flips: in every class that has one, the flip that comes first in
    # the greedy order must be a direct threshold crossing -- some higher-ranked
    # KEPT candidate of that class whose fp32 IoU with it lies on different sides of
    # nms_thres under the device's and the oracle's boxes, or a score-order swap;
    # later flips in the class can cascade from it
    unexplained = 0
    if flipped and common:
        ref_box = {}
        for r, bx in zip(common, ref_xyxy.numpy()):
            ref_box[r] = bx
        dev_box = {int(r): c[i, :4].numpy() for i, r in enumerate(rows)}
        ref_score = {r: float(np.float32(d0[r, 4]) * np.float32(cls_conf[r])) for r in common}
        dev_score = {int(r): float(scores[i]) for i, r in enumerate(rows)}
        cls_of = {int(r): int(cls[i]) for i, r in enumerate(rows)}
        for kcls in sorted({cls_of[r] for r in flipped if r in cls_of}):
            members = [r for r in common if cls_of.get(r) == kcls]
            order = sorted(members, key=lambda r: (-ref_score[r], r))
            rank = {r: i for i, r in enumerate(order)}
            first = min((r for r in flipped if cls_of.get(r) == kcls and r in rank), key=lambda r: rank[r])
            ref_kept = set(ref_rows.tolist())
            higher = [r for r in order[:rank[first]] if r in ref_kept]  # kept by both (all above `first` agree)
            dev_order = sorted(members, key=lambda r: (-dev_score[r], r))
            swapped = dev_order.index(first) != rank[first]

            def ious(boxes_of):
                a = np.asarray([boxes_of[r] for r in higher], np.float32).reshape(-1, 4)
                f = np.asarray(boxes_of[first], np.float32)
                with np.errstate(invalid='ignore', divide='ignore'):
                    w = np.maximum(np.float32(0), np.minimum(a[:, 2], f[2]) - np.maximum(a[:, 0], f[0]))
                    h = np.maximum(np.float32(0), np.minimum(a[:, 3], f[3]) - np.maximum(a[:, 1], f[1]))
                    inter = w * h
                    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
                    area_f = (f[2] - f[0]) * (f[3] - f[1])
                    return (inter / (area_a + area_f - inter)).astype(np.float64) > iou
            crossing = bool(np.any(ious(dev_box) != ious(ref_box))) if higher else False
            if not (crossing or swapped):
                unexplained += 1
    keep_flips = len(set(got.tolist()) ^ set(ref_rows[:max_det].tolist())) if k <= max_det else len(flipped)
    return dict(n_cand=len(dev_pass), n_cand_ref=len(ref_pass), member_flips=len(member),
                member_max_dist=max(boundary) if boundary else 0.0, box_maxdiff=box_maxdiff, cls_same=cls_same,
                nms_exact=bool(nms_exact), n_keep=k, n_keep_ref=len(ref_rows), keep_flips=keep_flips,
                unexplained_flips=unexplained)


def decoded_flip_report(dec_dev, dec_ref, nc, conf, iou):
    """Attribute every difference between the oracle's greedy chain (filter +
    per-class NMS, detect.py:98-137) run on two decoded tensors of ONE image --
    ``dec_dev`` from the device's forward, ``dec_ref`` from the oracle's -- to
    the forward's perturbation of scores and boxes:

      - ``member_flips``: rows that pass conf_thres on one side only; each must
        lie within ``max_score_delta`` of the threshold (``member_far`` counts
        those that do not);
      - keep flips: in every class with a differing keep decision, the flip
        that comes first in the oracle's greedy order must be caused directly:
        a membership flip at or above it, a score-order swap at or above it, or
        a kept higher-ranked box whose fp32 IoU with it lies on different sides
        of nms_thres under the two box sets (``unexplained_flips`` counts the
        classes where none holds; later flips of a class cascade from the
        first).
    Rows are compared by index, so both tensors must be (rows, 5 + nc) xywh."""
    from oracle import ref_post

    def prep(d):
        d = d.detach().to('cpu', torch.float32).clone()
        xyxy = torch.stack([d[:, 0] - d[:, 2] / 2, d[:, 1] - d[:, 3] / 2,
                            d[:, 0] + d[:, 2] / 2, d[:, 1] + d[:, 3] / 2], 1)
        cc, ci = torch.max(d[:, 5:5 + nc], 1)
        return xyxy.numpy(), (d[:, 4] * cc).numpy(), ci.numpy()

    bd, sd_, cd = prep(dec_dev)
    br, sr, cr = prep(dec_ref)
    kd = ref_post.nms_keep_rows(dec_dev.detach().to('cpu', torch.float32).clone().unsqueeze(0), nc, conf, iou)[0][0]
    kr = ref_post.nms_keep_rows(dec_ref.detach().to('cpu', torch.float32).clone().unsqueeze(0), nc, conf, iou)[0][0]
    kd, kr = set(kd.tolist()), set(kr.tolist())
    pd_, pr = set(np.flatnonzero(sd_ >= conf).tolist()), set(np.flatnonzero(sr >= conf).tolist())
    member = pd_ ^ pr
    union = sorted(pd_ | pr)
    delta = float(np.abs(sd_[union] - sr[union]).max()) if union else 0.0
    member_far = sum(1 for r in member if abs(float(sr[r]) - conf) > delta)
    cls_flips = sum(1 for r in union if cd[r] != cr[r])
    flipped = kd ^ kr

    def iou_gt(b, i, js):
        a = b[js].astype(np.float32).reshape(-1, 4)
        f = b[i].astype(np.float32)
        with np.errstate(invalid='ignore', divide='ignore'):
            w = np.maximum(np.float32(0), np.minimum(a[:, 2], f[2]) - np.maximum(a[:, 0], f[0]))
            h = np.maximum(np.float32(0), np.minimum(a[:, 3], f[3]) - np.maximum(a[:, 1], f[1]))
            inter = w * h
            den = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]) + (f[2] - f[0]) * (f[3] - f[1]) - inter
            return (inter / den).astype(np.float64) > iou

    unexplained, classes = 0, 0
    for k in sorted({int(cr[r]) for r in flipped} | {int(cd[r]) for r in flipped}):
        members = [r for r in union if int(cr[r]) == k or int(cd[r]) == k]
        cand_f = [r for r in flipped if r in members]
        if not cand_f:
            continue
        classes += 1
        order_r = sorted(members, key=lambda r: (-float(sr[r]), r))
        order_d = sorted(members, key=lambda r: (-float(sd_[r]), r))
        rank = {r: i for i, r in enumerate(order_r)}
        first = min(cand_f, key=lambda r: rank[r])
        pos = rank[first]
        above = order_r[:pos]
        if any(r in member or cd[r] != cr[r] for r in above + [first]):
            continue  # a membership / class flip at or above it changes the greedy input
        if order_d[:pos + 1] != order_r[:pos + 1]:
            continue  # a score-order swap at or above it
        higher = [r for r in above if r in kr]  # kept by both chains (all decisions above agree)
        if higher and bool(np.any(iou_gt(bd, first, higher) != iou_gt(br, first, higher))):
            continue  # an IoU threshold crossing against a kept higher-ranked box
        unexplained += 1
    return dict(n_pass_dev=len(pd_), n_pass_ref=len(pr), member_flips=len(member), member_far=member_far,
                max_score_delta=delta, cls_flips=cls_flips, n_keep_dev=len(kd), n_keep_ref=len(kr),
                keep_flips=len(flipped), flip_classes=classes, unexplained_flips=unexplained)


# ---- exact-operand parity (tests/test_gpu_conv_exact.py) ----
# Operands and bias that are small dyadic rationals make every product and every partial sum of a
# convolution exactly representable in fp32, so the fp32 accumulator holds the true sum whatever the
# order of the additions, and the stored element must be RNE(true sum) bit for bit.
# torch.float8_e4m3fn (OCP e4m3fn, tests/test_gpu_fp8_exact.py) is an element type here too: sign and
# seven magnitude bits, codes 0x7F / 0xFF are NaN (never expected, never accepted), no infinities. The
# +-448 clamp of an e4m3 store is the caller's job: rne refuses a value the cast would turn into NaN.
E4M3 = torch.float8_e4m3fn
_ELT_INT = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32, E4M3: torch.int8}
_ELT_MAG = {torch.int8: 0x7F, torch.int16: 0x7FFF, torch.int32: 0x7FFFFFFF}
_NAN_DISTANCE = 1 << 16  # elt_ulps of an e4m3 NaN code: farther than any two finite codes


def dyadic(shape, lo, hi, step, gen):
    """float64 tensor of uniformly drawn multiples of ``step`` in [lo, hi] (lo, hi multiples of step)."""
    k_lo, k_hi = round(lo / step), round(hi / step)
    assert k_lo * step == lo and k_hi * step == hi
    return torch.randint(k_lo, k_hi + 1, tuple(shape), generator=gen).double() * step


def e4m3_is_nan(t):
    """Mask of the NaN codes (0x7F, 0xFF) of an e4m3 tensor (or of its uint8 bytes)."""
    return (t.contiguous().view(torch.uint8) & 0x7F) == 0x7F


def rne(t64, dtype):
    """The reference element: torch's CPU cast of the float64 value (round to nearest, ties to even).
    The cast goes through fp32; that is one rounding for every value fp32 holds exactly (all the
    exact-operand sums), and otherwise moves the result only for a value within 2^-24 relative of
    a rounding boundary. e4m3: the value must already be clamped to +-448."""
    r = t64.to(torch.float64).to(dtype)
    if dtype == E4M3:
        assert not e4m3_is_nan(r).any(), "rne(e4m3): clamp the reference to +-448 first"
    return r


def _elt_key(t):
    """Sign-magnitude bit pattern -> an integer that counts representable values in order."""
    it = _ELT_INT[t.dtype]
    bits = t.contiguous().view(it).to(torch.int64)
    mag = bits & _ELT_MAG[it]
    return torch.where(bits < 0, -mag, mag)


def _elt_from_key(key, dtype):
    it = _ELT_INT[dtype]
    top = _ELT_MAG[it] + 1
    bits = torch.where(key < 0, (-key) | top, key)
    bits = torch.where(bits >= top, bits - 2 * top, bits)  # two's complement of the sign bit
    return bits.to(it).view(dtype)


def elt_ulps(got, ref, dtype):
    """Signed distance got - ref in representable values of ``dtype`` (+0 and -0 coincide). e4m3: ref
    holds no NaN code, and a NaN code in got is _NAN_DISTANCE away from everything."""
    assert got.dtype == dtype and ref.dtype == dtype
    d = _elt_key(got) - _elt_key(ref)
    if dtype == E4M3:
        assert not e4m3_is_nan(ref).any(), "an e4m3 NaN code is never expected"
        d = torch.where(e4m3_is_nan(got), torch.full_like(d, _NAN_DISTANCE), d)
    return d


def elt_neighbours(t64, dtype):
    """(below, above) as float64: the representable values of ``dtype`` that bracket t64
    (both equal to t64 where it is representable). e4m3: |t64| <= 448 (rne asserts it), so neither
    neighbour is ever the NaN code."""
    r = rne(t64, dtype)
    k, r64 = _elt_key(r), r.double()
    if dtype == E4M3:  # 448 has no finite neighbour above; it is only ever selected as itself
        up = _elt_from_key((k + 1).clamp(max=0x7E), dtype).double()
        dn = _elt_from_key((k - 1).clamp(min=-0x7E), dtype).double()
    else:
        up = _elt_from_key(k + 1, dtype).double()
        dn = _elt_from_key(k - 1, dtype).double()
    lo = torch.where(r64 <= t64, r64, dn)
    hi = torch.where(r64 >= t64, r64, up)
    return lo, hi


def rounding_stats(t64, dtype):
    """(share of elements not representable in ``dtype``, share that are exact ties between two
    adjacent representable values): what a store has to get right on these values."""
    lo, hi = elt_neighbours(t64, dtype)
    inexact = lo != hi
    tie = inexact & ((t64 - lo) == (hi - t64))
    return float(inexact.double().mean()), float(tie.double().mean())


# ---- the frame of the exact files (test_gpu_conv_exact.py, trio_case.py, test_gpu_stem_reorg.py) ----
# Outputs: the channel slice lies in the interior of a buffer pre-filled with a sentinel, and the whole
# buffer is compared, so a store before or after the slice, and an element left unwritten, show.
# Inputs: the channel slice lies between NaN channels and the tensor between NaN guards inside one
# allocation, so a read outside the operands reaches the output as NaN instead of as whatever the
# allocator left there. Padding weight rows and bias entries (cout .. cout_pad) hold grid values, so
# a padding channel that is stored lands as a value, not as the 0 a zero row computes.
SENTINEL = 3.0             # NHWC outputs: every element type represents it
SENTINEL_F32 = -6.0e23     # fp32 NCHW outputs: no reference comes near it
OUT_LEAD, OUT_TAIL = 16, 8  # NHWC output slice at channel 16 of a buffer 16 + cout + 8 wide
IN_LEAD, IN_TAIL = 8, 8     # input (and residual) slice at channel 8 of a buffer 8 + c + 8 wide
MIN_LIVE_PADDING = 0.90


def assert_bits(got, exp, what=""):
    """torch.equal on the bit patterns of two whole buffers; on a mismatch, how many elements and how far."""
    it = _ELT_INT[got.dtype]
    assert got.shape == exp.shape and got.dtype == exp.dtype, (got.shape, exp.shape, got.dtype, exp.dtype)
    gb, eb = got.contiguous().view(it), exp.contiguous().view(it)
    if torch.equal(gb, eb):
        return
    bad = gb != eb
    d = elt_ulps(got, exp, got.dtype)[bad]
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from RNE(true sum) or the "
                         f"sentinel; distance in representable values: min {int(d.min())}, max {int(d.max())}; "
                         f"{int(got.isnan().sum())} NaN; first at {[int(v) for v in bad.nonzero()[0]]}")


def out_frame(n, ho, wo, cout, dtype, lead=OUT_LEAD, tail=OUT_TAIL):
    """A sentinel-filled NHWC output buffer [n][ho][wo][lead + cout + tail]; the slice starts at ``lead``."""
    assert lead >= 0 and tail > 0
    return torch.full((n, ho, wo, lead + cout + tail), SENTINEL, dtype=dtype)


def expected_frame(elems_nhwc, lead=OUT_LEAD, tail=OUT_TAIL):
    """The whole expected buffer of out_frame: ``elems_nhwc`` (element type) in the slice, the sentinel outside."""
    n, ho, wo, c = elems_nhwc.shape
    exp = out_frame(n, ho, wo, c, elems_nhwc.dtype, lead, tail)
    exp[..., lead:lead + c] = elems_nhwc
    return exp


def out_planes(n, cout, ho, wo):
    """A sentinel-filled fp32 NCHW output buffer [n][cout + 2][ho][wo]: out_c_off 1, out_c_stride cout + 2."""
    return torch.full((n, cout + 2, ho, wo), SENTINEL_F32, dtype=torch.float32)


def expected_planes(ref_nchw):
    """The whole expected buffer of out_planes for an fp32 reference [n][cout][ho][wo]."""
    assert ref_nchw.dtype == torch.float32 and not bool((ref_nchw == SENTINEL_F32).any())
    n, c, ho, wo = ref_nchw.shape
    exp = out_planes(n, c, ho, wo)
    exp[:, 1:1 + c] = ref_nchw
    return exp


def nan_frame(t_nhwc, lead=IN_LEAD, tail=IN_TAIL):
    """[..., lead + c + tail] with ``t_nhwc`` at channel ``lead`` and NaN in every other channel."""
    c = t_nhwc.shape[-1]
    full = torch.full((*t_nhwc.shape[:-1], lead + c + tail), float('nan'), dtype=t_nhwc.dtype)
    full[..., lead:lead + c] = t_nhwc
    return full


def guard_elems(pad, w, row_elems, itemsize, align_bytes=16):
    """Elements of one NaN guard: at least (pad * w + pad + 1) * row_elems -- every position a tap of a
    pad-wide border can name before the first or after the last element, plus one -- rounded up so that
    the tensor behind it keeps ``align_bytes``. row_elems: in_c_stride (NHWC) or 1 (an NCHW image)."""
    a = align_bytes // itemsize
    return -(-((pad * w + pad + 1) * row_elems) // a) * a


def guarded(t, guard, device, fill=float('nan'), align_bytes=16):
    """``t`` (CPU, its final dtype) on ``device`` in the middle of ONE flat allocation, with ``guard``
    elements of ``fill`` (NaN for an input) before and after it. The guards are inside the allocation:
    nothing can fault, a read outside the tensor just becomes deterministic. Returns the view (it keeps
    the allocation alive)."""
    assert guard > 0 and (guard * t.element_size()) % align_bytes == 0
    flat = torch.full((2 * guard + t.numel(),), fill, dtype=t.dtype)
    flat[guard:guard + t.numel()] = t.reshape(-1)
    v = flat.to(device)[guard:guard + t.numel()].view(t.shape)
    assert v.data_ptr() % align_bytes == 0
    return v


OUT_GUARD = 1024  # elements of sentinel before and after an output buffer (a spilled padding channel of the
                  # last pixel, or a store in front of the first, stays inside the allocation and shows)


def guarded_out(t, device, guard=OUT_GUARD):
    """An output buffer ``t`` (CPU, pre-filled with its sentinel) on ``device`` between two guards of the
    same sentinel; fetch it with fetch_out, which also checks the guards."""
    return guarded(t, guard, device, fill=t.reshape(-1)[0].item())


def fetch_out(v, sentinel, guard=OUT_GUARD, what=""):
    """The CPU copy of a guarded_out buffer after the launch; asserts both guards still hold the sentinel."""
    flat = v._base.cpu()  # the flat allocation guarded() made
    assert v.storage_offset() == guard and flat.dim() == 1 and flat.numel() == 2 * guard + v.numel()
    for name, part in (("before", flat[:guard]), ("after", flat[guard + v.numel():])):
        assert bool((part == sentinel).all()), f"{what}: {int((part != sentinel).sum())} elements written {name} the buffer"
    return v.cpu()


def live_padding_share(pad_elems, sentinel):
    """Share of what the padding channels would store (``pad_elems``, already in the output's element
    type) whose bits differ from the sentinel they would land on; asserts >= MIN_LIVE_PADDING."""
    it = _ELT_INT[pad_elems.dtype]
    s = torch.full((1,), sentinel, dtype=pad_elems.dtype).view(it)
    assert pad_elems.numel() > 0
    share = float((pad_elems.contiguous().view(it) != s).double().mean())
    assert share >= MIN_LIVE_PADDING, f"padding channels: only {share:.3f} of their values differ from the sentinel"
    return share
