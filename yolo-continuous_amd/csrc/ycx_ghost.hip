// ycx_ghost_dw: GhostConv's second half and the Ghost shortcut in one launch, for gfx950.
//
// GhostConv.forward (nets/common.py:150-152) is cat[y, cv2(y)] with cv2 always the same conv:
// depthwise, 5x5, stride 1, pad 2. Ghost.forward (:244-245) adds a shortcut to that concat. This
// kernel reads the hidden map y (c channels) and writes the 2c-channel output:
//
//   out[.., j]     = y[.., j] (+ res[.., j])                                  j < c
//   out[.., c + j] = act(bias[j] + sum_ky sum_kx w[ky][kx][j] y[..]) (+ res[.., c + j])
//
// When y already sits in the first half of the output buffer (x == y, same slice) only the
// second half is stored: the plan places cv1's output there and no byte is copied.
//
// The generic grouped kernel (ycx_gconv.hip) stages a patch and fp32 weights in 64 KB of LDS and
// re-reads both per tap. Here nothing goes through LDS:
//
//   * a lane owns 2 channels of one output column and walks down a strip of output rows. Its
//     2 x 25 weights stay in registers (50 VGPRs) for the whole strip.
//   * lanes are numbered in memory order (channel pair fastest, then column), so a wave's load of
//     one pixel row is contiguous: 256 bytes of 16-bit data per 128 channels.
//   * input rows stream in ascending order. A lane loads the 5 columns of a row once, converts
//     them to fp32 once, and feeds the 5 output rows that row touches: five running accumulators
//     per channel, the oldest finished and stored after each row. The neighbours' overlapping
//     columns come from the vector L1, not from HBM.
//   * the next row's loads are issued before the current row's FMAs.
//   * accumulation order per output is kernel row, then kernel column, one fmaf per tap, taps
//     outside the image adding zero: the order ycx_conv2d_grouped documents, so on finite
//     operands the second half is bit-identical to that kernel's output.
//   * the first half (pass-through, or the shortcut add) comes from the centre column of the same
//     loaded row.
//
// No path reads outside [in_c_off, in_c_off + c) or outside the image, or writes outside
// [out_c_off, out_c_off + 2c).
#include <stdlib.h>

#include "ycx_internal.h"

// every fp32 operation below is written out: one fmaf per tap, one add for the bias, one for the
// residual. No contraction may merge the activation's multiply with the residual add.
#pragma clang fp contract(off)

namespace {

typedef __attribute__((ext_vector_type(2))) float f32x2;

struct HArgs {
  const void* x;
  const float* w;
  const float* bias;
  void* y;
  const void* res;
  int N, H, W, C, in_coff, in_cs, out_coff, out_cs, res_coff, res_cs;
  int act;
  float slope;
  int th, strips;   // output rows per strip, strips per image
  int inplace;      // the first half already sits in y: store the second half only
  unsigned total;   // lanes with work: N * strips * W * C / 2
};

template <typename T>
struct Pair {
  typedef __attribute__((ext_vector_type(2))) T type;
};

template <typename T>
__device__ __forceinline__ f32x2 widen(typename Pair<T>::type v) {
  return f32x2{(float)v[0], (float)v[1]};
}

template <typename T>
__device__ __forceinline__ typename Pair<T>::type narrow(f32x2 v) {
  typename Pair<T>::type o;
  o[0] = (T)v[0];  // round to nearest even
  o[1] = (T)v[1];
  return o;
}

template <typename T, bool RES>
__global__ __launch_bounds__(256) void ghost_dw_kernel(HArgs a) {
  typedef typename Pair<T>::type t2;
  constexpr bool FAST = sizeof(T) == 2;
  const unsigned t = blockIdx.x * 256u + threadIdx.x;
  if (t >= a.total) return;
  const unsigned P = (unsigned)a.C >> 1;
  unsigned r = t / P;
  const int c0 = (int)(t - r * P) * 2;
  const int x = (int)(r % (unsigned)a.W);
  r /= (unsigned)a.W;
  const int strip = (int)(r % (unsigned)a.strips);
  const int n = (int)(r / (unsigned)a.strips);
  const int y0 = strip * a.th;
  const int y1 = y0 + a.th < a.H ? y0 + a.th : a.H;

  f32x2 w[25];
#pragma unroll
  for (int tap = 0; tap < 25; ++tap) w[tap] = *reinterpret_cast<const f32x2*>(a.w + (size_t)tap * a.C + c0);
  const f32x2 bv = *reinterpret_cast<const f32x2*>(a.bias + c0);

  const T* xg = reinterpret_cast<const T*>(a.x) + a.in_coff + c0;
  T* yg = reinterpret_cast<T*>(a.y) + a.out_coff + c0;
  const T* rg = RES ? reinterpret_cast<const T*>(a.res) + a.res_coff + c0 : nullptr;
  const long long img = (long long)n * a.H;  // pixel (n, iy, ix) is (img + iy) * W + ix

  bool col_ok[5];
#pragma unroll
  for (int dx = 0; dx < 5; ++dx) col_ok[dx] = x + dx - 2 >= 0 && x + dx - 2 < a.W;

  // the 5 columns of input row iy, zero outside the image
  auto load_row = [&](int iy, t2 raw[5]) {
    const bool row_ok = iy >= 0 && iy < a.H;
    const long long pix = (img + iy) * a.W + x;
#pragma unroll
    for (int dx = 0; dx < 5; ++dx) {
      t2 v = t2{(T)0.0f, (T)0.0f};
      if (row_ok && col_ok[dx]) v = *reinterpret_cast<const t2*>(xg + (pix + dx - 2) * a.in_cs);
      raw[dx] = v;
    }
  };

  f32x2 acc[5];  // acc[ky]: output row iy + 2 - ky, which input row iy reaches with kernel row ky
#pragma unroll
  for (int ky = 0; ky < 5; ++ky) acc[ky] = f32x2{0.0f, 0.0f};

  t2 nxt[5];
  load_row(y0 - 2, nxt);
  for (int iy = y0 - 2; iy <= y1 + 1; ++iy) {
    t2 cur[5];
#pragma unroll
    for (int dx = 0; dx < 5; ++dx) cur[dx] = nxt[dx];
    if (iy < y1 + 1) load_row(iy + 1, nxt);  // in flight under this row's FMAs

    if (!a.inplace && iy >= y0 && iy < y1) {  // first half of output row iy: the centre column
      const long long pix = (img + iy) * a.W + x;
      if constexpr (RES) {
        const f32x2 rv = widen<T>(*reinterpret_cast<const t2*>(rg + pix * a.res_cs));
        *reinterpret_cast<t2*>(yg + pix * a.out_cs) = narrow<T>(widen<T>(cur[2]) + rv);
      } else {
        *reinterpret_cast<t2*>(yg + pix * a.out_cs) = cur[2];
      }
    }

    if (iy >= 0 && iy < a.H) {
      f32x2 xv[5];
#pragma unroll
      for (int dx = 0; dx < 5; ++dx) xv[dx] = widen<T>(cur[dx]);
#pragma unroll
      for (int ky = 0; ky < 5; ++ky)
#pragma unroll
        for (int kx = 0; kx < 5; ++kx) acc[ky] = __builtin_elementwise_fma(xv[kx], w[ky * 5 + kx], acc[ky]);
    }

    const int oy = iy - 2;  // kernel row 4 was its last: output row oy is complete
    if (oy >= y0) {
      const long long pix = (img + oy) * a.W + x;
      f32x2 v;
      v[0] = ycx_act<FAST>(acc[4][0] + bv[0], a.act, a.slope);
      v[1] = ycx_act<FAST>(acc[4][1] + bv[1], a.act, a.slope);
      if constexpr (RES) v = v + widen<T>(*reinterpret_cast<const t2*>(rg + pix * a.res_cs + a.C));
      *reinterpret_cast<t2*>(yg + pix * a.out_cs + a.C) = narrow<T>(v);
    }
#pragma unroll
    for (int ky = 4; ky > 0; --ky) acc[ky] = acc[ky - 1];
    acc[0] = f32x2{0.0f, 0.0f};
  }
}

template <typename T>
ycx_status launch_t(const HArgs& a, unsigned nwg, hipStream_t st) {
  if (a.res)
    hipLaunchKernelGGL((ghost_dw_kernel<T, true>), dim3(nwg), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((ghost_dw_kernel<T, false>), dim3(nwg), dim3(256), 0, st, a);
  return ycx_launch_status();
}

// Development A/B only: YCX_GHOST_TH=<rows> fixes the strip height.
int forced_th() {
  static const int v = [] {
    const char* s = getenv("YCX_GHOST_TH");
    return s ? atoi(s) : 0;
  }();
  return v;
}

}  // namespace

extern "C" ycx_status ycx_ghost_dw(const ycx_conv_desc* d, const void* x, const float* w, const float* bias, void* y,
                                   const void* residual, void* stream) {
  YCX_CHECK_ARG(d);  // the descriptor is judged before the data pointers (checked below, before the launch)
  YCX_CHECK_ARG(d->n > 0 && d->h > 0 && d->w > 0 && d->cin > 0 && d->cout > 0 && d->ho > 0 && d->wo > 0);
  YCX_CHECK_ARG(d->kh > 0 && d->kw > 0 && d->stride > 0 && d->pad >= 0 && d->groups > 0);
  YCX_CHECK_ARG(d->in_c_off >= 0 && d->in_c_off + d->cin <= d->in_c_stride);
  YCX_CHECK_ARG(d->out_c_off >= 0 && d->out_c_off + d->cout <= d->out_c_stride);
  YCX_CHECK_ARG(d->ho == (d->h + 2 * d->pad - d->kh) / d->stride + 1);
  YCX_CHECK_ARG(d->wo == (d->w + 2 * d->pad - d->kw) / d->stride + 1);
  YCX_CHECK_ARG(!residual || (d->res_c_off >= 0 && d->res_c_off + d->cout <= d->res_c_stride));
  YCX_CHECK_SUPPORTED(d->kh == 5 && d->kw == 5 && d->stride == 1 && d->pad == 2);
  YCX_CHECK_SUPPORTED(d->groups == d->cin && d->cout == 2 * d->cin);
  YCX_CHECK_SUPPORTED(d->dtype == YCX_DT_BF16 || d->dtype == YCX_DT_F16 || d->dtype == YCX_DT_F32);
  YCX_CHECK_SUPPORTED(d->act == YCX_ACT_NONE || d->act == YCX_ACT_SILU || d->act == YCX_ACT_LEAKY);
  YCX_CHECK_SUPPORTED(d->out_layout == YCX_OUT_NHWC && !d->in_pool && d->k_split <= 1);
  // channel fields in multiples of 8, the granularity of every slice the plan makes
  YCX_CHECK_SUPPORTED(d->cin % 8 == 0 && d->in_c_off % 8 == 0 && d->in_c_stride % 8 == 0 && d->out_c_off % 8 == 0 &&
                      d->out_c_stride % 8 == 0);
  if (residual) YCX_CHECK_SUPPORTED(d->res_c_off % 8 == 0 && d->res_c_stride % 8 == 0);
  YCX_CHECK_SUPPORTED((long long)d->n * d->h * d->w < (1LL << 31));
  YCX_CHECK_ARG(x && w && bias && y);
  int inplace = 0;
  if (x == y) {
    if (d->in_c_off == d->out_c_off && d->in_c_stride == d->out_c_stride) {
      YCX_CHECK_ARG(!residual);  // the add would overwrite halo pixels that neighbours still read
      inplace = 1;
    } else {  // another slice of the same buffer: only if the channel ranges are disjoint
      YCX_CHECK_ARG(d->in_c_stride == d->out_c_stride);
      YCX_CHECK_ARG(d->in_c_off + d->cin <= d->out_c_off || d->out_c_off + d->cout <= d->in_c_off);
    }
  }

  // Strip height: the tallest of 32, 16, 8, 4 rows (evened out over the image) that still gives
  // the chip about three waves per SIMD; a taller strip re-reads fewer halo rows and loads its
  // weights once for more rows.
  const long long per_row = (long long)d->n * d->w * (d->cin / 2);
  static const int heights[4] = {32, 16, 8, 4};
  int th = 0, strips = 0;
  for (int cand : heights) {
    if (forced_th() > 0) cand = forced_th();
    strips = (d->h + cand - 1) / cand;
    th = (d->h + strips - 1) / strips;
    strips = (d->h + th - 1) / th;
    if (per_row * strips >= 3000LL * 64 || forced_th() > 0) break;
  }
  const long long total = per_row * strips;
  YCX_CHECK_SUPPORTED(total < (1LL << 31) - 256);
  HArgs a;
  a.x = x; a.w = w; a.bias = bias; a.y = y; a.res = residual;
  a.N = d->n; a.H = d->h; a.W = d->w; a.C = d->cin; a.in_coff = d->in_c_off; a.in_cs = d->in_c_stride;
  a.out_coff = d->out_c_off; a.out_cs = d->out_c_stride; a.res_coff = d->res_c_off; a.res_cs = d->res_c_stride;
  a.act = d->act; a.slope = d->leaky_slope;
  a.th = th; a.strips = strips; a.inplace = inplace; a.total = (unsigned)total;
  const unsigned nwg = (unsigned)((total + 255) / 256);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  switch (d->dtype) {
    case YCX_DT_BF16: return launch_t<__bf16>(a, nwg, st);
    case YCX_DT_F16: return launch_t<_Float16>(a, nwg, st);
    default: return launch_t<float>(a, nwg, st);
  }
}
