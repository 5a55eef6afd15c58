/*
 * ycx.h — C ABI of libycx_hip.so, the MI355X (gfx950) YOLO inference hot path.
 *
 * Every entry point is `extern "C"`, takes plain pointers/sizes, returns an
 * int32 status (0 = OK) and launches asynchronously on the caller's HIP
 * stream (passed as `void*`, i.e. a hipStream_t). The library never allocates
 * device memory on the hot path: activations, packed weights, workspaces and
 * outputs are owned by the caller (PyTorch's caching allocator in the Python
 * host package).
 *
 * Reference interfaces each entry point replaces (xin-pu/yolo-continuous):
 *   ycx_conv2d          Conv.forward = act(bn(conv2d(x)))      nets/common.py:97-109
 *                       RepConv.forward (re-parameterised)      nets/common.py:477-495
 *                       Detect head 1x1 convs (bias, no act)    nets/detect.py:27-38
 *                       IDetect conv + ImplicitA/M (folded)     nets/idetect.py:26-31
 *   ycx_conv2d_grouped  Conv with g > 1 (small groups, depthwise) nets/common.py:97-109
 *                       dw_conv                                 nets/common.py:20-22
 *                       RobustConv2's strided depthwise half     nets/common.py:132
 *   ycx_deconv2d        nn.ConvTranspose2d, kernel == stride     nets/common.py:133-134 (RobustConv2)
 *   ycx_ghost_dw        GhostConv's cat[y, cv2(y)], cv2 depthwise 5x5  nets/common.py:142-152
 *                       Ghost's conv(x) + shortcut(x) on that concat   nets/common.py:233-245
 *   ycx_stem_conv       first Conv on the fp32 NCHW image       nets/common.py:105-106 (Cin=3)
 *   ycx_stem_conv2      first two Convs fused (3->32, then 3x3   cfg/net/yolov7.yaml:7-8,
 *                       stride 2 -> 64); the stem output stays   nets/common.py:97-109
 *                       in LDS
 *   ycx_stem_conv_reorg ReOrg + the Conv that reads it (P6 stems)   nets/common.py:43-51, 97-109
 *   ycx_maxpool         MP / SP / SPPCSPC max-pools             nets/common.py:25-40, 257
 *   ycx_copy_channels   nn.Upsample(None, 2, 'nearest')         cfg/net/yolov7.yaml:71,85
 *                       Concat (only when a slice cannot alias)  nets/common.py:54-60
 *   ycx_space_depth     Contract, Expand                         nets/common.py:787-812
 *                       Focus's pixel-phase cat on an activation nets/common.py:767
 *   ycx_classify        Classify: AdaptiveAvgPool2d(1) + Conv2d  nets/common.py:815-825
 *                       (its centre tap) + Flatten
 *   ycx_decode          decode_box (one head level)             detect.py:29-87
 *   ycx_filter_decoded  non_max_suppression lines 98-121        detect.py:98-121
 *   ycx_decode_filter   decode_box + the same filter, fused     detect.py:29-121
 *   ycx_conv2d_head     Detect head conv (one level) fused with  nets/detect.py:27-38 +
 *                       decode_box + the candidate filter        detect.py:29-121
 *   ycx_idetect_decode  IDetect eval branch (strides supplied)  nets/idetect.py:33-45
 *   ycx_ibin_decode     IBin eval branch (strides supplied)     nets/ibin.py:48-72,
 *                                                                losses/sigmoid_bin.py:49-63
 *   ycx_sort_nms        per-class torchvision.ops.nms loop      detect.py:124-137
 *   ycx_run_ops         Model.forward layer loop                nets/yolo.py:143-153
 *   ycx_letterbox       image -> network input                   detect.py:16-26,
 *                                                                image_enhance/letter_box.py:27-60
 *   ycx_correct_boxes   yolo_correct_boxes on the NMS output     detect.py:139-165
 */
#ifndef YCX_H_
#define YCX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The version stays 9 across the `groups` field appended to ycx_conv_desc (and the
 * ycx_conv2d_grouped / YCX_OP_GCONV additions) and across ycx_deconv2d / YCX_OP_DECONV and
 * ycx_ghost_dw / YCX_OP_GHOST, which each add
 * an entry point and an op kind but no struct and no field: the library and its ctypes mirror
 * (ycx/_lib.py) are always built together in-tree and check each other's struct sizes
 * (ycx_struct_size, ids 0 to 11 unchanged) at load time; a zero-initialised descriptor
 * means what it meant before. ycx_space_depth / YCX_OP_DEPTH add ycx_depth_desc, a new member of
 * ycx_op's union that is smaller than `pair`, so sizeof(ycx_op) and the ids 0 to 11 stay as they are;
 * the new struct has no id (the ctypes mirror is checked through sizeof(ycx_op)). ycx_classify /
 * YCX_OP_CLASSIFY add ycx_classify_desc in the same way: a union member smaller than `pair`, no id. */
#define YCX_ABI_VERSION 9

typedef int32_t ycx_status;
enum {
  YCX_OK = 0,
  YCX_ERR_BAD_ARG = 1,      /* null pointer, negative size, inconsistent shape  */
  YCX_ERR_UNSUPPORTED = 2,  /* shape/dtype the kernels do not implement          */
  YCX_ERR_LAUNCH = 3,       /* hipGetLastError() after a launch was not success   */
  YCX_ERR_CAPACITY = 4      /* workspace / output capacity too small              */
};

/* YCX_DT_FP8: OCP e4m3fn activations and weights (CDNA4 block-scaled MFMA with
 * unit block scales, fp32 accumulate). Each activation buffer carries one
 * power-of-two scale s (stored byte = e4m3(clamp(v * s, +-448))); weights
 * carry one per output channel (see ycx_conv_desc).
 * YCX_DT_F16: IEEE half activations and weights, fp32 accumulate: the bf16
 * kernels on the f16 MFMA (same rate, 11-bit significand): the precision mode
 * that holds north_star's 1e-3 at bf16 speed. Activations must stay below
 * 65504 in magnitude (fp16 range). */
enum { YCX_DT_BF16 = 0, YCX_DT_F32 = 1, YCX_DT_FP8 = 2, YCX_DT_F16 = 3 };
/* YCX_ACT_SILU_PS: SiLU of a conv whose packed weights and bias were pre-multiplied by
 * k = -log2(e) (fp8: the fp32 bias and dequantisation rows instead), so the epilogue holds
 * c' = k c and computes silu(c) = c' / (k (1 + 2^c')) = c' * rcp(fma(2^c', k, k)) -- one
 * exp, one fma, one rcp and one multiply per value instead of a multiply more (r06). The
 * 16-bit and fp8 kernels; not the fp32 parity path. */
enum { YCX_ACT_NONE = 0, YCX_ACT_SILU = 1, YCX_ACT_LEAKY = 2, YCX_ACT_SILU_PS = 3 };
enum {
  YCX_OUT_NHWC = 0,       /* activation dtype, [N][Ho][Wo][out_c_stride] at out_c_off         */
  YCX_OUT_NCHW_F32 = 1,   /* fp32 [N][out_c_stride][Ho][Wo] at out_c_off (Detect raw logits)   */
  YCX_OUT_NHWC_UP2 = 2    /* activation dtype, each pixel written to its 2x2 block of a
                             [N][2Ho][2Wo][out_c_stride] buffer (conv fused with nearest x2)   */
};

/* Convolution: NHWC activations, weights packed [cout_pad][kh][kw][cin] in the
 * activation dtype, fp32 bias[cout_pad] (BN folded in). groups = 1 (field `groups` 0 or 1).
 * YCX_DT_FP8: weight rows are zero-padded to a multiple of 128 bytes
 * ([cout_pad][ceil(kh*kw*cin / 128) * 128] e4m3 of w * s_w[co]); bias points
 * to fp32 [2 * cout_pad]: the bias, then dq[co] = 1 / (s_w[co] * s_x); the
 * epilogue computes act(acc * dq + bias) (+ residual * res_scale) and stores
 * e4m3(clamp(v * out_scale)) (fp32 NCHW head outputs: unscaled). The stem
 * (ycx_stem_conv) reads the fp32 image with fp32 weights and only its output
 * is e4m3 (out_scale). cout_pad % 64 == 0 and cin in {32, 64, 128k}.
 * Channel slices: x, y and the residual are slices of wider buffers, in_c_off + cin <= in_c_stride,
 * out_c_off + cout <= out_c_stride (YCX_OUT_NCHW_F32: out_c_off is the first of cout planes), and the
 * residual's res_c_off + cout <= res_c_stride. 16-byte channel vectors: in_c_off and in_c_stride are
 * multiples of 8 (16-bit), 4 (f32) or 16 (fp8); for the NHWC layouts cout, out_c_off and out_c_stride
 * are multiples of 8, as are res_c_off and res_c_stride; YCX_OUT_NCHW_F32 has no such rule (cout 255).
 * cin is a multiple of the tile's K step, so no entry point reads a channel outside
 * [in_c_off, in_c_off + cin), nor a pixel outside the tensor: whatever lies there, NaN included,
 * never reaches an output.
 * Padded output channels: rows cout .. cout_pad of w and entries cout .. cout_pad of bias may hold any
 * finite values, not only zeros (the zero padding promised above is the fp8 rows' K padding alone).
 * They are computed and never stored: no entry point writes outside [out_c_off, out_c_off + cout) of
 * a pixel (of the planes, for YCX_OUT_NCHW_F32). tests/test_gpu_conv_exact.py holds every dense kernel
 * to both rules with NaN around the inputs, sentinels around the outputs and live padding rows. */
typedef struct ycx_conv_desc {
  int32_t n, h, w, cin, in_c_off, in_c_stride;
  int32_t ho, wo, cout, cout_pad, out_c_off, out_c_stride;
  int32_t kh, kw, stride, pad;
  int32_t act;              /* YCX_ACT_*                                           */
  float leaky_slope;        /* for YCX_ACT_LEAKY (0.1 in yolov7-tiny.yaml)          */
  int32_t dtype;            /* YCX_DT_*: activations & weights                     */
  int32_t out_layout;       /* YCX_OUT_*                                            */
  int32_t res_c_off, res_c_stride; /* residual (same dtype/shape as the output)   */
  int32_t tile;             /* 0 = auto, else a tile id (see ycx_conv_tile_name)    */
  float out_scale;          /* YCX_DT_FP8 only: output quantisation scale          */
  float res_scale;          /* YCX_DT_FP8 only: residual dequantisation (1 / s_res) */
  int32_t in_pool;          /* 1: x is the (2h, 2w) map that MP's k2 s2 max-pool reduces to the
                             * (h, w) input (nets/common.py:25-31), pooled in the conv's operand
                             * staging (1x1/s1/p0: 16-bit with cin % 64 == 0, or YCX_DT_FP8
                             * with cin % 128 == 0, r04), the same pool as ycx_maxpool: in 16-bit a NaN
                             * in a window makes its pooled pixel NaN in every output channel;
                             * 0: x is the input */
  int32_t k_split;          /* > 1: the K loop (kh*kw*cin) is cut into k_split contiguous ranges run by
                             * separate workgroups, whose fp32 partial sums go to a caller-owned
                             * workspace (ycx_conv2d_ws, ycx_conv_workspace_size) and are summed in a
                             * fixed order by a second launch (bias, act, residual, store): deterministic.
                             * 16-bit LDS-DMA tiles only (16, 18, 56), r06. 0 or 1: no split */
  int32_t groups;           /* 0 or 1: dense. > 1: only ycx_conv2d_grouped takes it (below); every other
                             * entry point returns YCX_ERR_UNSUPPORTED */
} ycx_conv_desc;

/* Max-pool, NHWC, torch.nn.MaxPool2d semantics, floor mode. The pad value is -inf, so a window
 * never comes out below its inputs (a border window of negative values keeps its negative
 * maximum). NaN propagates as in torch: a 16-bit or fp32 window that holds a NaN gives NaN,
 * whatever else it holds (the 16-bit range guard relies on it: inf / NaN must reach the heads
 * through a bare MP / SP too). The sign of a zero maximum is not specified.
 * YCX_DT_FP8: input and output share one scale (max commutes with it). e4m3 activations hold
 * neither NaN (codes 0x7F / 0xFF) nor infinities: the fp8 stores saturate and cannot produce
 * them, so the result for such a code is unspecified. */
typedef struct ycx_pool_desc {
  int32_t n, h, w, c, in_c_off, in_c_stride;
  int32_t ho, wo, out_c_off, out_c_stride;
  int32_t k, stride, pad;
  int32_t dtype;
  /* levels > 1: a cascade of `levels` identical 'same' pools (stride 1, pad k/2) in one
   * launch, pool i of pool i-1 (SPPCSPC's 5/9/13 as 5, 5o5, 5o5o5: nets/common.py:257),
   * level i written to channels out_c_off + i*c of y. 0 or 1: one pool. */
  int32_t levels;
} ycx_pool_desc;

/* Channel-slice copy with optional nearest x2 upsample (scale = 1 or 2).
 * out_layout YCX_OUT_NHWC keeps the dtype; YCX_OUT_NCHW_F32 writes fp32
 * [N][out_c_stride][Ho][Wo] (a model output that is not a Detect head). */
typedef struct ycx_copy_desc {
  int32_t n, h, w, c, in_c_off, in_c_stride;
  int32_t out_c_off, out_c_stride;
  int32_t scale;
  int32_t dtype;
  int32_t out_layout;
  float dequant;            /* YCX_DT_FP8 with YCX_OUT_NCHW_F32: 1 / s_in (else unused) */
} ycx_copy_desc;

/* Space <-> depth move between two NHWC channel slices (ycx_space_depth, below). n, h, w, c describe
 * the input slice, ho, wo the output map; the output slice is c * gain^2 (Contract, Focus) or
 * c / gain^2 (Expand) channels wide. */
enum { YCX_SD_CONTRACT = 0, YCX_SD_EXPAND = 1, YCX_SD_FOCUS = 2 };
typedef struct ycx_depth_desc {
  int32_t n, h, w, c, in_c_off, in_c_stride;
  int32_t ho, wo, out_c_off, out_c_stride;
  int32_t gain;             /* s, 2 .. 4 (YCX_SD_FOCUS: 2)                          */
  int32_t mode;             /* YCX_SD_*                                             */
  int32_t dtype;            /* YCX_DT_*: moved as bytes                             */
} ycx_depth_desc;

/* Global average pool + dense layer over an NHWC channel slice (ycx_classify, below). n, h, w, c describe
 * the input slice; the output is fp32 [n][cout]. */
typedef struct ycx_classify_desc {
  int32_t n, h, w, c, in_c_off, in_c_stride;
  int32_t cout;
  int32_t dtype;            /* YCX_DT_*: the input's element type                   */
  float dequant;            /* YCX_DT_FP8: 1 / s_in, as ycx_copy_desc (else unused) */
} ycx_classify_desc;

/* Decode of one head level (detect.py:29-87 semantics). head is fp32 NCHW
 * [n][na*no][h][w]; out is fp32 [n][rows_total][no], written at row_off.
 * anchors_scaled[2a], [2a+1] = anchor_w/stride_w, anchor_h/stride_h computed in
 * double and rounded to fp32 exactly as detect.py:43-44 does. */
typedef struct ycx_decode_desc {
  int32_t n, h, w, na, no;
  int32_t rows_total, row_off;
  float anchors_scaled[16];
} ycx_decode_desc;

/* One NMS candidate (32 bytes): normalised xyxy box, objectness, best class
 * confidence, best class id, row index into the concatenated [rows_total]. */
typedef struct ycx_cand {
  float x1, y1, x2, y2;
  float obj, cls_conf;
  int32_t cls, row;
} ycx_cand;

/* Filter of a decoded [n][rows][no] tensor (detect.py:98-121): xywh -> xyxy in
 * place, class max (first index on ties), score = obj*cls_conf >= conf_thres. */
typedef struct ycx_filter_desc {
  int32_t n, rows, no, nc;
  float conf_thres;         /* compared in fp32, as torch does for a float32 tensor */
  int32_t write_xyxy;       /* 1: mutate pred[..., :4] to xyxy like detect.py:103  */
} ycx_filter_desc;

/* Fused decode + filter straight from the three fp32 NCHW head tensors. */
typedef struct ycx_decode_filter_desc {
  int32_t n, nl, na, no, nc;
  int32_t h[4], w[4];       /* per level, in head order (P5, P4, P3 for Detect)    */
  int32_t row_off[4];       /* first row of each level in the concatenated rows    */
  int32_t rows_total;
  float anchors_scaled[4][16];
  float conf_thres;
} ycx_decode_filter_desc;

/* Per-image, per-class greedy NMS with torchvision.ops.nms semantics. */
typedef struct ycx_nms_desc {
  int32_t n, rows_total, nc;
  int32_t max_det;          /* output rows per image (padded); counts are not capped */
  double iou_thres;         /* compared as (double)iou > iou_thres, like torchvision */
} ycx_nms_desc;

/* Letterbox of one uint8 HWC image (BGR kept, as detect.py feeds it) into an
 * fp32 CHW network input: bilinear resize to new_h x new_w (half-pixel
 * centres, edge clamp, float64 weights, round-half-even to uint8), content at
 * (top, left) of out_h x out_w, border value `pad`, then value / 255 in fp32.
 * The host computes the geometry (round(w r) etc.) like letter_box.py. */
typedef struct ycx_letterbox_desc {
  int32_t h0, w0, c;          /* source image (c <= 4)                     */
  int32_t src_row_stride;     /* bytes between source rows (>= w0 * c)     */
  int32_t out_h, out_w;       /* letterboxed size                          */
  int32_t new_h, new_w;       /* resized content size                      */
  int32_t top, left;          /* content offset                            */
  int32_t pad;                /* border value, 114 in the reference        */
} ycx_letterbox_desc;

/* yolo_correct_boxes (detect.py:139-165) applied in place to the padded NMS
 * output dets[n][max_det][7]: rows 0..min(counts[i], max_det) become
 * [y1, x1, y2, x2] in original-image pixels (float64 math, stored fp32, as
 * numpy does). image_hw: [n][2] int32 original (h, w) per image. */
typedef struct ycx_correct_desc {
  int32_t n, max_det;
  int32_t input_h, input_w;   /* network input size                        */
  int32_t letterbox;          /* letterbox_image flag                      */
} ycx_correct_desc;

/* Decode + candidate filter of one Detect head level, fused into the head's
 * 1x1 conv (ycx_conv2d_head): the fp32 logits of a tile never leave the CU.
 * Candidates are the same as ycx_decode_filter's for this level (same float
 * operations in the same order): rows row_off + a * h * w + cell. */
typedef struct ycx_head_desc {
  int32_t na, no, nc;           /* anchors, outputs per anchor (nc + 5), classes      */
  int32_t rows_total, row_off;  /* candidate rows per image (all levels), this level's */
  float conf_thres;             /* obj * cls_conf >= conf_thres, compared in fp32     */
  float anchors_scaled[16];     /* as ycx_decode_desc                                 */
} ycx_head_desc;

/* A pre-built op for ycx_run_ops (the static execution plan of Model.forward). */
enum { YCX_OP_CONV = 1, YCX_OP_STEM = 2, YCX_OP_POOL = 3, YCX_OP_COPY = 4, YCX_OP_STEM2 = 5, YCX_OP_HEAD = 6,
       YCX_OP_CONV_PAIR = 7,
       YCX_OP_STEM_REORG = 8 /* ycx_stem_conv_reorg: d.conv, in, weight, bias, out */,
       YCX_OP_GCONV = 9 /* ycx_conv2d_grouped: d.conv, in, weight (fp32), bias, out, residual */,
       YCX_OP_DECONV = 10 /* ycx_deconv2d: d.conv, in, weight, bias, out */,
       YCX_OP_GHOST = 11 /* ycx_ghost_dw: d.conv, in, weight (fp32), bias, out, residual */,
       YCX_OP_DEPTH = 12 /* ycx_space_depth: d.depth, in, out */,
       YCX_OP_CLASSIFY = 13 /* ycx_classify: d.classify, in, weight (fp32), bias, out, workspace */ };
typedef struct ycx_op {
  int32_t kind;
  int32_t pad_;
  union {
    ycx_conv_desc conv;
    ycx_pool_desc pool;
    ycx_copy_desc copy;
    ycx_depth_desc depth;   /* DEPTH                                                 */
    ycx_classify_desc classify;  /* CLASSIFY                                         */
    ycx_conv_desc pair[2];  /* STEM2: [0] the stem, [1] the stride-2 conv it feeds;
                               CONV_PAIR: [0] the first 1x1 conv, [1] the 1x1 conv reading it */
    struct {
      ycx_conv_desc conv;
      ycx_head_desc head;
    } head;                 /* HEAD: the head conv and its level's decode           */
  } d;
  const void* in;           /* x                                                    */
  const void* weight;       /* packed weights (conv/stem; STEM2: the stem's)        */
  const float* bias;        /* bias (conv/stem; STEM2: the stem's)                  */
  void* out;                /* y                                                    */
  const void* residual;     /* optional residual (conv)                             */
  const void* weight2;      /* STEM2 / CONV_PAIR: the second conv's packed weights  */
  const float* bias2;       /* STEM2 / CONV_PAIR: the second conv's bias            */
  void* cand;               /* HEAD: ycx_cand [n][rows_total]                      */
  int32_t* cand_rows;       /* HEAD: [n][rows_total]                                */
  int32_t* cand_counts;     /* HEAD: [n], zeroed before the first level's op        */
  int32_t* status;          /* HEAD (nullable): the range guard flag, below         */
  void* out2;               /* CONV_PAIR: the second conv's output (out: the first's, nullable) */
  void* workspace;          /* CONV with d.conv.k_split > 1: fp32 partials, >= ycx_conv_workspace_size;
                               CLASSIFY: fp32 [n][c], the pooled means                */
  /* CONV_PAIR with out3 set: ycx_conv2d_pair_pool, the pair plus the pooled 1x1 `conv3` */
  ycx_conv_desc conv3;
  const void* weight3;      /* conv3's packed weights                               */
  const float* bias3;       /* conv3's bias                                         */
  void* out3;               /* conv3's output; null: a plain pair                   */
} ycx_op;

int ycx_abi_version(void);
/* sizeof() of the ABI structs, so FFI mirrors can verify their layout:
 * 0 conv_desc, 1 pool_desc, 2 copy_desc, 3 decode_desc, 4 cand, 5 filter_desc,
 * 6 decode_filter_desc, 7 nms_desc, 8 op, 9 letterbox_desc, 10 correct_desc,
 * 11 head_desc.
 * Returns 0 for an unknown id. */
size_t ycx_struct_size(int32_t which);
const char* ycx_strerror(ycx_status s);
const char* ycx_conv_tile_name(int32_t tile);
/* The tile ycx_conv2d uses for d->tile == 0. d->res_c_stride > 0 means the
 * call will pass a residual (tile 22, the weight-resident 1x1, takes none). */
int32_t ycx_conv_pick_tile(const ycx_conv_desc* d);
/* Introspection (host only, no device call): the (output-channel tile, pixel
 * tile) that workgroup `bid` of an LDS-DMA conv launch of nwg = n_ct * n_pt
 * workgroups computes under channel-group count gc (the XCD region map), as
 * ct * 65536 + pt; -1 on bad arguments. Lets tests prove the map bijective. */
int32_t ycx_conv_tile_of(int32_t bid, int32_t nwg, int32_t n_ct, int32_t gc);

ycx_status ycx_conv2d(const ycx_conv_desc* d, const void* x, const void* w,
                      const float* bias, void* y, const void* residual, void* stream);
/* Grouped convolution, d->groups > 1 (Conv with g > 1, nets/common.py:97-109; dw_conv, :20-22):
 * direct NHWC conv, VALU FMA with fp32 accumulation in a fixed order (kernel row, kernel column,
 * input channel of the group), for the small groups the MFMA tiles cannot take:
 *   cin_g = cin / groups == cout_g = cout / groups, cin_g in {1, 2, 4, 8, 16} (1: depthwise);
 *   kh == kw in {3, 5, 7}, stride 1 or 2, pad == kh / 2; dtype bf16 / fp16 / f32;
 *   depthwise only (cin_g == 1) also kh == kw == 11 and stride 4 or 8 (RobustConv2's strided half,
 *   nets/common.py:128-132: [32, 7, 4], [32, 11, 8]), any of k in {3, 5, 7, 11} with any of s in {1, 2, 4, 8}.
 * x, y, residual: NHWC channel slices as ycx_conv2d (in_c_*, out_c_*, res_c_*; offsets, strides and
 * cout multiples of 8: a lane owns a 16-byte vector of 16-bit channels); cout_pad and tile are not used.
 * w: fp32 in every dtype, [kh][kw][cout][cin_g], unscaled; bias: fp32 [cout].
 * y = act(acc + bias) (+ residual), act YCX_ACT_NONE / SILU / LEAKY; 16-bit stores round to nearest
 * even. Only YCX_OUT_NHWC, no in_pool, no k_split, no YCX_ACT_SILU_PS, no fp8: YCX_ERR_UNSUPPORTED,
 * as is any other shape. Null pointers and inconsistent shapes (ho / wo, a slice past its stride,
 * cin % groups != 0): YCX_ERR_BAD_ARG before any device call. The descriptor is judged before the data
 * pointers: a null x / w / bias / y reports YCX_ERR_BAD_ARG only with a descriptor the kernel takes. */
ycx_status ycx_conv2d_grouped(const ycx_conv_desc* d, const void* x, const float* w, const float* bias,
                              void* y, const void* residual, void* stream);
/* Transposed convolution with kernel == stride (nn.ConvTranspose2d(cin, cout, s, s, padding 0,
 * output_padding 0, dilation 1, groups 1, bias), nets/common.py:133-134): the learned x-s upsample,
 *   y[n][oh][ow][co] = act(bias[co] + sum_ci x[n][oh / s][ow / s][ci] * W[ci][co][oh % s][ow % s]).
 * d is a ycx_conv_desc with kh == kw == stride == s in {2, 4, 8}, pad == 0, ho == h * s, wo == w * s,
 * groups 0 or 1; cout_pad, tile and the res_* fields are not used. The windows do not overlap, so this
 * is one GEMM (rows s*s*cout, columns n*h*w, K = cin) whose tiles are stored straight to their s x s
 * output blocks: no intermediate reaches memory.
 * x, y: NHWC channel slices as ycx_conv2d (in_c_*, out_c_*; cin, cout, offsets and strides multiples
 * of 8: 16-byte vectors), so y may be a slice of a concat buffer.
 * w: packed [s*s][cout][cin] in the activation dtype (bf16 / fp16 / f32), tap = (oh % s) * s + (ow % s),
 *    i.e. torch's weight[ci][co][dy][dx] permuted (2, 3, 1, 0); bias: fp32 [cout]. Unscaled: a SiLU
 *    epilogue is the plain YCX_ACT_SILU.
 * 16-bit: MFMA with fp32 accumulation over ci in a fixed order; f32: one fmaf per ci, ascending.
 * act YCX_ACT_NONE / SILU / LEAKY; 16-bit stores round to nearest even.
 * YCX_ERR_BAD_ARG before any device call: null pointers, n <= 0, ho / wo not h * s / w * s, a slice
 * past its stride. YCX_ERR_UNSUPPORTED: kh != stride, s not in {2, 4, 8}, pad != 0, fp8,
 * YCX_ACT_SILU_PS, an out_layout other than YCX_OUT_NHWC, in_pool, k_split > 1, groups > 1,
 * cin % 8, cout % 8 or a channel offset / stride that is no multiple of 8. The descriptor is judged
 * before the data pointers, as in ycx_conv2d_grouped. */
ycx_status ycx_deconv2d(const ycx_conv_desc* d, const void* x, const void* w, const float* bias, void* y,
                        void* stream);
/* GhostConv's output cat[y, cv2(y)] (nets/common.py:150-152), cv2 the depthwise 5x5 / stride 1 / pad 2
 * conv every GhostConv has, optionally plus Ghost's shortcut (:244-245) over all 2c channels:
 *   out[.., j]     = x[.., j] (+ res[.., j])                                                   j < c
 *   out[.., c + j] = act(bias[j] + sum_ky sum_kx w[ky][kx][j] * x[n][oy + ky - 2][ox + kx - 2][j]) (+ res[.., c + j])
 * d: cin = c (the hidden map), cout = 2c, groups = c, kh == kw == 5, stride 1, pad 2, ho == h, wo == w;
 * dtype bf16 / fp16 / f32, YCX_OUT_NHWC; cout_pad and tile are not used. x, y, residual: NHWC channel
 * slices (in_c_*, out_c_*, res_c_*; c, offsets and strides multiples of 8); the output and residual
 * slices are 2c wide. w: fp32 [5][5][c], the bytes of ycx_conv2d_grouped's [kh][kw][cout][1], unscaled;
 * bias: fp32 [c].
 * The first half without a residual is a bit copy; with one, an fp32 add rounded once to the element
 * type (nearest even). The second half accumulates in fp32, one fmaf per tap in the order kernel row,
 * kernel column, taps outside the image adding zero: the order of ycx_conv2d_grouped, so on finite
 * operands it is bit-identical to that kernel. act YCX_ACT_NONE / SILU (plain) / LEAKY.
 * In place: x == y with in_c_off == out_c_off and in_c_stride == out_c_stride means the first half
 * already sits where it belongs; only the second half is stored. In place with a residual, or x == y
 * with any other intersecting channel ranges: YCX_ERR_BAD_ARG.
 * YCX_ERR_BAD_ARG before any device call: null pointers, inconsistent shapes (ho / wo), a slice past its
 * stride. YCX_ERR_UNSUPPORTED: any other k, stride, pad or groups, cout != 2 cin, fp8, YCX_ACT_SILU_PS,
 * in_pool, k_split > 1, another out_layout, a channel field that is no multiple of 8. The descriptor is
 * judged before the data pointers, as in ycx_conv2d_grouped. */
ycx_status ycx_ghost_dw(const ycx_conv_desc* d, const void* x, const float* w, const float* bias, void* y,
                        const void* residual, void* stream);
/* ycx_conv2d with a caller-owned workspace for d->k_split > 1 (split-K: fp32 partials of
 * every K range, then one reduce launch; ycx_conv2d itself returns YCX_ERR_CAPACITY for
 * k_split > 1). ycx_conv_workspace_size: the bytes it needs (0 without a split). */
size_t ycx_conv_workspace_size(const ycx_conv_desc* d);
ycx_status ycx_conv2d_ws(const ycx_conv_desc* d, const void* x, const void* w, const float* bias, void* y,
                         const void* residual, void* workspace, size_t workspace_bytes, void* stream);
/* The K split the library recommends for this conv on the tile it picks (1: none). */
int32_t ycx_conv_pick_ksplit(const ycx_conv_desc* d);
/* Detect head 1x1 conv of one level (bf16, act none, cout = na * no <= 256,
 * out_layout YCX_OUT_NCHW_F32) fused with that level's decode + filter: appends
 * the passing rows to cand / cand_rows / cand_counts exactly as
 * ycx_decode_filter does. `heads` (nullable) also receives the raw fp32 NCHW
 * logits [n][cout][ho][wo] (the compat Model.forward output).
 * `status` (nullable, one int32 the caller zeroes): set to YCX_HEAD_NONFINITE when
 * any logit of the launch is inf or NaN -- the fp16 plan's range guard (an
 * activation past 65504 becomes inf at its producer's store and reaches the heads
 * as inf / NaN). Never cleared by the library. No reference counterpart: the
 * reference computes in fp32 (nets/yolo.py:143-153). */
enum { YCX_HEAD_NONFINITE = 1 };
ycx_status ycx_conv2d_head(const ycx_conv_desc* d, const ycx_head_desc* h, const void* x, const void* w,
                           const float* bias, float* heads, ycx_cand* cand, int32_t* cand_rows,
                           int32_t* cand_counts, int32_t* status, void* stream);
/* Two chained 1x1 / stride-1 convs in one launch (Conv, nets/common.py:97-109, twice):
 * ya = act_a(W_a x + b_a) (cin 64 / 128 / 256 -> cout 256, `ya` nullable: then it is
 * not stored) and yb = act_b(W_b ya + b_b) (256 -> cout_pad 128 or 256), where `b` reads
 * nothing but `a`'s output: the yolov7 160^2 ELAN exit (layer 11 -> layer 14,
 * cfg/net/yolov7.yaml). The intermediate stays on chip (one HBM read of it saved);
 * outputs bit-identical to two ycx_conv2d calls with the weight-resident 1x1 (tile 22).
 * NHWC 16-bit (d->dtype bf16 / fp16), channel slices as ycx_conv2d. */
ycx_status ycx_conv2d_pair(const ycx_conv_desc* a, const ycx_conv_desc* b, const void* x, const void* w_a,
                           const float* bias_a, void* ya, const void* w_b, const float* bias_b, void* yb,
                           void* stream);
/* ycx_conv2d_pair plus the 1x1 conv of the MP branch that also reads `a`'s output:
 * yc = act_c(W_c MP(ya) + b_c) (256 -> cout_pad 128, cout % 8 == 0), MP the k2 s2 max-pool
 * (nets/common.py:25-31), pooled from the ya tile on chip: yolov7 layers 11 -> 14 and
 * 11 -> 12 -> 13. With `ya` null the 256-channel map is neither written nor read back.
 * `c` is the descriptor ycx_conv2d would take for the pooled conv (c->in_pool == 1,
 * c->h == a->h / 2, c->w == a->w / 2, c->cin == 256; its in_c_* are not used). The launch
 * walks tiles of two image rows x 32 columns: a->h % 2 == 0 and a->w % 32 == 0.
 * YCX_ERR_UNSUPPORTED otherwise. ya / yb as ycx_conv2d_pair; yc bit-identical to
 * ycx_conv2d(c) on the stored ya. */
ycx_status ycx_conv2d_pair_pool(const ycx_conv_desc* a, const ycx_conv_desc* b, const ycx_conv_desc* c,
                                const void* x, const void* w_a, const float* bias_a, void* ya, const void* w_b,
                                const float* bias_b, void* yb, const void* w_c, const float* bias_c, void* yc,
                                void* stream);
/* Stem conv: fp32 NCHW input (the model input, cin <= 4), weights fp32
 * [kh][kw][cin][cout_pad], output NHWC in d->dtype. in_c_* describe the NCHW
 * channel count (in_c_stride = channels of the input tensor). */
ycx_status ycx_stem_conv(const ycx_conv_desc* d, const float* x, const float* w,
                         const float* bias, void* y, void* stream);
/* The stem (3x3, stride 1 or 2, pad 1, 3 -> 32, bf16 NHWC result kept in LDS)
 * followed by a 3x3 / stride-2 / pad-1 conv 32 -> cout (cout_pad 64) that
 * consumes only it: one kernel, the 32-channel stem map never reaches HBM.
 * `stem` and `conv` are the two layers' own descriptors (conv->h/w = the stem
 * output size); conv output as for ycx_conv2d (NHWC bf16, channel slice).
 * Requires conv->ho % 4 == 0, conv->wo % 32 == 0 and stem->act == conv->act.
 * dtype YCX_DT_FP8 (both descriptors): the pair still computes in bf16 with
 * bf16 w_conv and plain bias; only the output is e4m3 (conv->out_scale). */
ycx_status ycx_stem_conv2(const ycx_conv_desc* stem, const ycx_conv_desc* conv, const float* x,
                          const float* w_stem, const float* b_stem, const void* w_conv,
                          const float* b_conv, void* y, void* stream);
/* First Conv of a network whose layer 0 is ReOrg (nets/common.py:43-51, then :97-109): the
 * space-to-depth is done in the operand gather, the 4C-channel map never exists in memory
 * (a 3x3 / s / pad-1 conv over ReOrg(x) is a 6x6 / 2s / pad-2 conv over x).
 * x: fp32 NCHW image [n][C][2h][2w] (8-byte aligned), C = d->in_c_stride <= 4, d->in_c_off == 0.
 * d describes the conv as the reference sees it AFTER ReOrg: d->h, d->w the reorganised map,
 * d->cin == 4*C, kh == kw == 3, pad 1, stride 1 or 2.
 * w: fp32 [kh][kw][cin][cout_pad], cin in ReOrg's channel order q*C + c with
 *    q = 0 (even row, even col), 1 (odd row, even col), 2 (even row, odd col), 3 (odd row, odd col).
 * y, dtype, act, out_c_*, out_scale: as ycx_stem_conv (bf16 / fp16 / f32 / fp8 output, NHWC;
 * cout_pad 32 or a multiple of 64; f32: the exact fp32 FMA chain of the parity mode). */
ycx_status ycx_stem_conv_reorg(const ycx_conv_desc* d, const float* x, const float* w,
                               const float* bias, void* y, void* stream);
ycx_status ycx_maxpool(const ycx_pool_desc* d, const void* x, void* y, void* stream);
ycx_status ycx_copy_channels(const ycx_copy_desc* d, const void* x, void* y, void* stream);
/* Space <-> depth on an NHWC activation: Contract and Expand (nets/common.py:787-812) and the pixel-phase
 * concat inside Focus.forward (:767), a pure move between two channel slices (the in_c_* / out_c_*
 * convention of ycx_copy_channels, so y may be a slice of a concat buffer). s = d->gain, C = d->c:
 *   YCX_SD_CONTRACT  y [n][h/s][w/s][s*s*C]:        y[n, ho, wo, (a*s+b)*C + c] = x[n, ho*s+a, wo*s+b, c]
 *   YCX_SD_EXPAND    y [n][h*s][w*s][C'], C' = C/(s*s): y[n, h*s+a, w*s+b, c'] = x[n, h, w, (a*s+b)*C' + c']
 *   YCX_SD_FOCUS     y [n][h/2][w/2][4C], s == 2:   y[n, ho, wo, (2*b+a)*C + c] = x[n, 2*ho+a, 2*wo+b, c]
 * Expand is the inverse of Contract. In Focus the row phase varies fastest: the C-channel blocks come in
 * the order (a, b) = (0,0), (1,0), (0,1), (1,1), ReOrg's order (ycx_stem_conv_reorg).
 * dtype bf16 / fp16 / f32 / fp8, moved as 2-, 2-, 4- and 1-byte elements: NaN payloads, -0.0 and every
 * e4m3 code pass through unchanged; fp8 input and output share one scale. The contiguous channel run
 * (C for Contract and Focus, C' for Expand) and every channel offset and stride are multiples of 8
 * elements. Each lane moves one vector of up to 16 bytes; consecutive lanes store consecutive output
 * vectors (the store side is fully coalesced, the load side reads whole runs); a grid-stride loop over a
 * 64-bit flat index; no LDS.
 * YCX_ERR_BAD_ARG before any device call: null pointers, n <= 0, h % s or w % s non-zero (Contract,
 * Focus), C % (s*s) non-zero (Expand), ho / wo not what h, w and s imply, a slice past its stride,
 * x == y unless the two slices have one pixel stride and disjoint channel ranges.
 * YCX_ERR_UNSUPPORTED: a gain outside 2 .. 4, Focus with s != 2, a run, offset or stride that is no
 * multiple of 8, an unknown dtype or mode. The descriptor is judged before the data pointers, as in
 * ycx_conv2d_grouped. */
ycx_status ycx_space_depth(const ycx_depth_desc* d, const void* x, void* y, void* stream);
/* Classify (nets/common.py:815-825) on an NHWC activation: AdaptiveAvgPool2d(1), the Conv2d on the 1 x 1
 * map it leaves, Flatten. With an odd kernel and p == k // 2 only the centre tap of that conv meets data, so
 * the layer is  y[n, o] = bias[o] + sum_c w[o, c] * mean_hw x[n, :, :, c].
 *   x          the channel slice [in_c_off, in_c_off + c) of an NHWC buffer with in_c_stride channels,
 *              dtype bf16 / fp16 / f32 / fp8 (e4m3; the mean is multiplied by d->dequant = 1 / s_in)
 *   w          fp32 [cout][c], the centre tap, in every precision (as ycx_conv2d_grouped's weights)
 *   bias       fp32 [cout], nullable
 *   y          fp32 [n][cout]
 *   workspace  fp32 [n][c]: receives the pooled means
 * Two launches on the stream, one op. The pool: each lane reads 16 bytes of consecutive channels (8 bytes
 * for an e4m3 slice on 8- but not 16-channel bounds), a block of 256 threads covers CL channel vectors
 * x 256 / CL pixel phases, every lane sums its pixels in fp32 in ascending order, the phases are combined
 * through LDS in ascending order, then one IEEE division by h * w. The linear step: one wave per output
 * and up to eight images, lanes over c with 16-byte loads, fp32 FMAs, a fixed xor-butterfly over the
 * lanes. No atomics: two runs on the same input give the same bits. The launch sizes are functions of the
 * descriptor alone.
 * YCX_ERR_BAD_ARG before any device call: a null descriptor, x, w, y or workspace; an unknown dtype;
 * n, h, w, c or cout <= 0; c, in_c_off or in_c_stride no multiple of 8; in_c_off < 0 or
 * in_c_off + c > in_c_stride.
 * YCX_ERR_UNSUPPORTED, also before any device call: h * w >= 2^24 (the divisor and the pixel index stay exact),
 * more than 2^31 - 1 pool blocks, or n > 8 * 65535 (the linear step's grid). */
ycx_status ycx_classify(const ycx_classify_desc* d, const void* x, const float* w, const float* bias, float* y,
                        float* workspace, void* stream);
/* fp32 -> OCP e4m3fn bytes: y[i] = e4m3(clamp(x[i] * scale, +-448)), round to
 * nearest even: the exact cast of the YCX_DT_FP8 epilogues (calibration checks). */
ycx_status ycx_quantize_fp8(const float* x, void* y, int64_t n, float scale, void* stream);

ycx_status ycx_decode(const ycx_decode_desc* d, const float* head, float* out, void* stream);
/* IDetect's eval outputs for one level (nets/idetect.py:33-45): xview gets the
 * raw map as (n, na, h, w, no); z [n][rows_total][no] gets, at row_off, the
 * decoded rows xy = (sigmoid*2 - 0.5 + grid) * stride, wh = (sigmoid*2)^2 *
 * anchor (pixels; d->anchors_scaled holds the level's anchor_grid in pixels).
 * The reference leaves IDetect.stride unset (its eval raises); the caller
 * supplies it. */
ycx_status ycx_idetect_decode(const ycx_decode_desc* d, float stride, const float* head, float* z, float* xview,
                              void* stream);
/* IBin's eval outputs for one level (nets/ibin.py:48-72): as ycx_idetect_decode, but width and
 * height come from SigmoidBin.forward (losses/sigmoid_bin.py:49-63) instead of (sigmoid*2)^2.
 * d->no is the raw width nc + 3 + 2*(bin_count + 1): x, y, then for w and for h one regression
 * logit and bin_count bin logits, then objectness and the classes. head: fp32 NCHW
 * [n][na*no][h][w]; xview gets the raw map as (n, na, h, w, no); z [n][rows_total][nc + 5] gets,
 * at row_off, rows in (a, y, x) order with p = sigmoid(raw):
 *   xy = (p*2 - 0.5 + grid) * stride
 *   w  = clamp((p[2]*2 - 1) * (float)(4.0/21) + w_bins[argmax p[3..23]], 0, 4) * anchor_w
 *   h  = the same from p[24], p[25..45] and h_bins, times anchor_h
 *   z[4..] = p[46..]
 * The arg-max is torch.max's: the first index of the maximum of the sigmoid'd scores.
 * w_bins, h_bins: HOST arrays of bin_count floats (the modules' `bins` buffers), copied into the
 * kernel's arguments. d->anchors_scaled holds the level's anchor_grid in pixels. Cells per block
 * are derived from no so that the two LDS tiles stay inside 64 KB.
 * The descriptor is judged before the data pointers. YCX_ERR_BAD_ARG: a null descriptor, a
 * non-positive size or bin_count, no <= 2*(bin_count+1) + 3 (no class), row_off < 0 or
 * row_off + na*h*w > rows_total, a null pointer. YCX_ERR_UNSUPPORTED: bin_count != 21 (the
 * reference's eval slices are written out for 21 bins), na > 8, no > 256, n > 65535. */
ycx_status ycx_ibin_decode(const ycx_decode_desc* d, float stride, int32_t bin_count, const float* w_bins,
                           const float* h_bins, const float* head, float* z, float* xview, void* stream);
/* Candidate outputs of both filters:
 *   cand        [n][rows] ycx_cand, written only at the rows that pass (dense by row)
 *   cand_rows   [n][rows] int32, the passing row indices, compacted (any order)
 *   cand_counts [n] int32, number of passing rows; MUST be zeroed before the call
 *               (the filters append with wave-aggregated atomics). */
ycx_status ycx_filter_decoded(const ycx_filter_desc* d, float* pred, ycx_cand* cand,
                              int32_t* cand_rows, int32_t* cand_counts, void* stream);
ycx_status ycx_decode_filter(const ycx_decode_filter_desc* d, const float* const* heads,
                             ycx_cand* cand, int32_t* cand_rows, int32_t* cand_counts, void* stream);
/* Device self-check behind the class scan of the decode filters (no reference
 * counterpart): adds to *violations (device uint64, caller-zeroed) the number of
 * adjacent finite-float pairs x < y with sigmoid(x) > sigmoid(y) for the
 * decoders' sigmoid, over every float, plus (r06) the floats m in [-80, 6] at
 * which sigmoid(m - max(|m|, 1) 2^-12) is not below sigmoid(m). The filters'
 * exact class argmax relies on it being 0 (ycx_internal.h, ycx_class_argmax and
 * the fast path of ycx_class_finish). */
ycx_status ycx_check_sigmoid_monotone(unsigned long long* violations, void* stream);
size_t ycx_nms_workspace_size(const ycx_nms_desc* d);
/* Sorts each image's candidates by (class asc, score desc, row asc) — the order
 * of detect.py:124-137 with a stable torchvision sort — and runs greedy NMS per
 * class. cand_rows must list each row at most once per image (both filters and the
 * fused head decode append every passing row exactly once): the class buckets are
 * counted per list entry and filled per distinct row. Outputs: dets [n][max_det][7] = x1,y1,x2,y2,obj,cls_conf,cls (fp32),
 * keep_rows [n][max_det] (row index, -1 padded), keep_counts [n] (not capped
 * by max_det; rows beyond max_det are dropped from dets/keep_rows). */
ycx_status ycx_sort_nms(const ycx_nms_desc* d, const ycx_cand* cand, const int32_t* cand_rows,
                        const int32_t* cand_counts, void* workspace, size_t workspace_bytes,
                        float* dets, int32_t* keep_rows, int32_t* keep_counts, void* stream);

ycx_status ycx_letterbox(const ycx_letterbox_desc* d, const uint8_t* src, float* dst, void* stream);
/* n same-sized images in one launch: image i is read at src + i * src_image_stride
 * bytes and written to dst + i * c * out_h * out_w (one NCHW fp32 batch): the
 * preprocessing of detect.py:16-26 for a whole batch (bench.py --image-in). */
ycx_status ycx_letterbox_batch(const ycx_letterbox_desc* d, int32_t n, int64_t src_image_stride,
                               const uint8_t* src, float* dst, void* stream);
ycx_status ycx_correct_boxes(const ycx_correct_desc* d, float* dets, const int32_t* counts,
                             const int32_t* image_hw, void* stream);

/* Run a static op list in order on one stream. If `events` is non-null it must
 * hold n_ops+1 hipEvent_t; event i is recorded before op i and event n_ops
 * after the last (per-op kernel timing for the roofline report). */
ycx_status ycx_run_ops(const ycx_op* ops, int32_t n_ops, void* stream, void* const* events);

/* 1: ycx_run_ops wraps every op in a roctx range "op<i> <kind> <tile> n HxW cin->cout k s"
 * (rocprofv3 --marker-trace); 0 (default): no tracing. The roctx library is dlopen'ed
 * on the first ycx_set_trace(1); YCX_ERR_UNSUPPORTED (tracing stays off) if it is
 * absent. No reference counterpart (its only instrument is the @timer decorator,
 * utils/helper_torch.py:10-20). */
ycx_status ycx_set_trace(int32_t on);
/* Kernel-side bounds checks (`make -C yolo-continuous_amd/csrc debug` builds
 * libycx_hip_dbg.so with -DYCX_DEBUG_BOUNDS; select it with YCX_LIB=<path>): every
 * conv epilogue store is tested against the output extent its descriptor implies and
 * skipped if outside. out[0] = violations since the last reset, out[1] = the first
 * offending source line. YCX_ERR_UNSUPPORTED from a release build. */
ycx_status ycx_debug_bounds(uint32_t* out, int32_t reset);
/* Capture ycx_run_ops into a HIP graph and instantiate it (graph_exec out). */
ycx_status ycx_graph_capture(const ycx_op* ops, int32_t n_ops, void* stream, void** graph_exec);
ycx_status ycx_graph_launch(void* graph_exec, void* stream);
ycx_status ycx_graph_destroy(void* graph_exec);

#ifdef __cplusplus
}
#endif
#endif /* YCX_H_ */
