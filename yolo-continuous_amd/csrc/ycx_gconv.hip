// ycx_conv2d_grouped: direct NHWC grouped / depthwise convolution for gfx950.
//
// Conv(c1, c2, k, s, g > 1) (nets/common.py:97-109) and dw_conv (:20-22) with
// cin_g == cout_g in {1, 2, 4, 8, 16}: a group that small has no MFMA tile, and the op is
// bandwidth-bound (a depthwise 3x3 does 9 MACs per element moved), so this is VALU FMA with
// fp32 accumulation shaped around the memory system:
//
//   * a workgroup (256 threads) owns TH x TW output pixels of one image and a chunk of
//     kChunk = 32 channels. The (TH-1)s+k by (TW-1)s+k input patch of that chunk is staged
//     once into LDS with 16-byte loads (zero-filled outside the image), so the k*k taps
//     re-read LDS, not HBM; the chunk's fp32 weights sit in LDS next to it (all taps when
//     they fit 16 KB, else one kernel row at a time).
//   * a lane owns 8 consecutive channels (one 16-byte vector of 16-bit data) of up to
//     four output pixels; because cin_g divides 8 (or is 16), the input channels those 8
//     outputs read are the same 8 (or the surrounding 16) channels.
//   * accumulation order is fixed: kernel row, kernel column, input channel of the group,
//     one fmaf each, so the fp32 parity mode is reproducible run to run.
//   * epilogue act(acc + bias) (+ residual), converted with the hardware's
//     round-to-nearest-even casts and written as 16-byte vector stores.
//
// Depthwise only (cin_g == 1): also k = 11 and stride 4 or 8, RobustConv2's strided half
// (nets/common.py:128-132: [32, 5, 2], [32, 7, 4], [32, 11, 8]). The staged patch of a T x T output
// tile is ((T - 1) s + k)^2 pixels of 32 channels, and the 48 KB patch buffer holds 768 pixels of
// 16-bit data, 384 of fp32: at s = 8, k = 11 the smallest tile the s <= 2 table offers (1 x 8:
// 11 x 67 pixels) fits 16-bit only, and its square tiles are far out of reach (8 x 8: 67 x 67). So
// strides 4 and 8 pick from a table of their own, 8 x 4 down to 1 x 1 outputs: at s = 4, k = 7 that
// is 8 x 4 (35 x 19) in 16-bit and 4 x 4 (19 x 19) in fp32, at s = 8, k = 11 it is 4 x 2 (35 x 19)
// and 2 x 2 (19 x 19). The windows of such a conv barely overlap (3 pixels of 11 at s = 8), so a small
// tile costs little halo: 35 x 19 staged for 32 x 16 used. Every (k, s, g) with s <= 2 keeps its table,
// its tile and its instantiation.
#include "ycx_internal.h"

namespace {

constexpr int kChunk = 32;          // channels per workgroup
constexpr int kLanesPerPx = 4;      // 8-channel vectors per chunk
constexpr int kSlots = 4;           // output pixels per lane (64 pixel lanes x 4 = 256-pixel tile at most)
constexpr int kXBytes = 48 * 1024;  // LDS: input patch
constexpr int kWFloats = 4096;      // LDS: weights (16 KB)

struct GArgs {
  const void* x;
  const float* w;
  const float* bias;
  void* y;
  const void* res;
  int N, H, W, C, in_coff, in_cs;
  int Ho, Wo, out_coff, out_cs, res_coff, res_cs;
  int S, P, act;
  float slope;
  int th, tw_log2, ih, iw;    // tile: th x (1 << tw_log2) outputs, ih x iw staged inputs
  int tiles_x, tiles_y, n_chunks;
  int wrows;                  // kernel rows of weights resident in LDS at a time (K or 1)
};

template <typename T>
__device__ __forceinline__ void load8(const T* p, float v[8]) {
  if constexpr (sizeof(T) == 2) {
    typedef __attribute__((ext_vector_type(8))) T tx8;
    const tx8 r = *reinterpret_cast<const tx8*>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)r[j];
  } else {
    const f32x4 r0 = *reinterpret_cast<const f32x4*>(p), r1 = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] = r0[j]; v[4 + j] = r1[j]; }
  }
}

template <typename T>
__device__ __forceinline__ void store8(T* p, const float v[8]) {
  if constexpr (sizeof(T) == 2) {
    typedef __attribute__((ext_vector_type(8))) T tx8;
    tx8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (T)v[j];  // round to nearest even
    *reinterpret_cast<tx8*>(p) = o;
  } else {
    *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(p + 4) = f32x4{v[4], v[5], v[6], v[7]};
  }
}

// T: element type; K: kernel size; G: channels per group (cin_g == cout_g).
template <typename T, int K, int G>
__global__ __launch_bounds__(256) void gconv_kernel(GArgs a) {
  constexpr int XV = G == 16 ? 16 : 8;  // input channels a lane reads per tap
  __shared__ __attribute__((aligned(16))) unsigned char xs_raw[kXBytes];
  __shared__ __attribute__((aligned(16))) float ws[kWFloats];
  T* xs = reinterpret_cast<T*>(xs_raw);

  const int tid = threadIdx.x;
  int b = blockIdx.x;
  const int chunk = b % a.n_chunks;
  b /= a.n_chunks;
  const int txi = b % a.tiles_x;
  b /= a.tiles_x;
  const int tyi = b % a.tiles_y;
  const int n = b / a.tiles_y;
  const int c_base = chunk * kChunk;
  const int tw = 1 << a.tw_log2;
  const int oy0 = tyi * a.th, ox0 = txi * tw;
  const int iy0 = oy0 * a.S - a.P, ix0 = ox0 * a.S - a.P;

  // ---- stage the input patch: [ih][iw][kChunk] elements, 16-byte vectors ----
  {
    constexpr int EV = 16 / (int)sizeof(T);  // elements per 16-byte vector
    constexpr int VPP = kChunk / EV;         // vectors per pixel
    const int total = a.ih * a.iw * VPP;
    const T* xg = reinterpret_cast<const T*>(a.x);
    for (int i = tid; i < total; i += 256) {
      const int pix = i / VPP, v = i - pix * VPP;
      const int r = pix / a.iw, cx = pix - r * a.iw;
      const int iy = iy0 + r, ix = ix0 + cx, ch = c_base + v * EV;
      uint4 val = make_uint4(0u, 0u, 0u, 0u);
      if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W && ch < a.C)
        val = *reinterpret_cast<const uint4*>(xg + ((size_t)(n * a.H + iy) * a.W + ix) * a.in_cs + a.in_coff + ch);
      *reinterpret_cast<uint4*>(xs + (size_t)i * EV) = val;
    }
  }

  const int cv = tid & (kLanesPerPx - 1);  // this lane's 8-channel vector of the chunk
  const int pl = tid >> 2;                 // pixel lane 0..63
  const int c0 = c_base + cv * 8;
  const int npx = a.th << a.tw_log2;
  const int xc = G == 16 ? (cv >> 1) * 16 : cv * 8;  // first input channel (within the chunk) this lane reads

  int sp[kSlots];  // LDS pixel index of each slot's window origin, -1: no such pixel in the tile
#pragma unroll
  for (int s = 0; s < kSlots; ++s) {
    const int p = pl + 64 * s;
    const int py = p >> a.tw_log2, px = p & (tw - 1);
    sp[s] = p < npx ? (py * a.S) * a.iw + px * a.S : -1;
  }

  float acc[kSlots][8];
#pragma unroll
  for (int s = 0; s < kSlots; ++s)
#pragma unroll
    for (int o = 0; o < 8; ++o) acc[s][o] = 0.0f;

  // LDS weights: [row][kw][cv][j][o], o the lane's 8 outputs, j the input channel of the group
  const int wr = a.wrows;
  for (int ky0 = 0; ky0 < K; ky0 += wr) {
    if (ky0) __syncthreads();  // the previous rows' weights have been read
    {
      const int per_row = K * kChunk * G;  // floats of one kernel row of this chunk
      const int total = wr * per_row;
      for (int i = tid; i < total; i += 256) {
        // global [kh][kw][cout][cin_g]: i enumerates (row, kw, c_local, j)
        const int j = i % G, t = i / G, cl = t % kChunk, tap = t / kChunk;  // tap = row * K + kw
        const int c = c_base + cl;
        const float v = c < a.C ? a.w[((size_t)(ky0 * K + tap) * a.C + c) * G + j] : 0.0f;
        ws[((tap * kLanesPerPx + (cl >> 3)) * G + j) * 8 + (cl & 7)] = v;
      }
    }
    __syncthreads();  // weights (and, first time, the input patch) are in LDS
    // one tap: the slots' input vectors, then per input channel of the group 8 weights and 8 FMAs per slot
    auto tap = [&](int kr, int kx) {
      {
        const int ky = ky0 + kr;
        float xv[kSlots][XV];
#pragma unroll
        for (int s = 0; s < kSlots; ++s) {
          if (sp[s] >= 0) {
            const T* p = xs + (size_t)(sp[s] + ky * a.iw + kx) * kChunk + xc;
            load8<T>(p, xv[s]);
            if constexpr (XV == 16) load8<T>(p + 8, xv[s] + 8);
          } else {
#pragma unroll
            for (int j = 0; j < XV; ++j) xv[s][j] = 0.0f;
          }
        }
        const float* wt = ws + (size_t)((kr * K + kx) * kLanesPerPx + cv) * G * 8;
#pragma unroll
        for (int j = 0; j < G; ++j) {
          const f32x4 w0 = *reinterpret_cast<const f32x4*>(wt + j * 8);
          const f32x4 w1 = *reinterpret_cast<const f32x4*>(wt + j * 8 + 4);
#pragma unroll
          for (int s = 0; s < kSlots; ++s)
#pragma unroll
            for (int o = 0; o < 8; ++o) {
              const int xi = G == 16 ? j : (o / G) * G + j;  // input channel of output o's group
              acc[s][o] = __builtin_fmaf(xv[s][xi], o < 4 ? w0[o] : w1[o - 4], acc[s][o]);
            }
        }
      }
    };
    // depthwise: the K taps of a row unrolled (independent LDS reads in flight); wider groups keep one tap's
    // operands live at a time (unrolled, they spill: 16 inputs x 4 slots per tap)
    for (int kr = 0; kr < wr; ++kr) {
      if constexpr (G == 1) {
#pragma unroll
        for (int kx = 0; kx < K; ++kx) tap(kr, kx);
      } else {
#pragma unroll 1
        for (int kx = 0; kx < K; ++kx) tap(kr, kx);
      }
    }
  }

  // ---- epilogue ----
  if (c0 >= a.C) return;
  float bv[8];
  load8<float>(a.bias + c0, bv);
#pragma unroll
  for (int s = 0; s < kSlots; ++s) {
    const int p = pl + 64 * s;
    const int oy = oy0 + (p >> a.tw_log2), ox = ox0 + (p & (tw - 1));
    if (p >= npx || oy >= a.Ho || ox >= a.Wo) continue;
    const size_t pix = (size_t)(n * a.Ho + oy) * a.Wo + ox;
    float v[8];
#pragma unroll
    for (int o = 0; o < 8; ++o) v[o] = ycx_act<sizeof(T) == 2>(acc[s][o] + bv[o], a.act, a.slope);
    if (a.res) {
      float rv[8];
      load8<T>(reinterpret_cast<const T*>(a.res) + pix * a.res_cs + a.res_coff + c0, rv);
#pragma unroll
      for (int o = 0; o < 8; ++o) v[o] += rv[o];
    }
    store8<T>(reinterpret_cast<T*>(a.y) + pix * a.out_cs + a.out_coff + c0, v);
  }
}

template <typename T, int K>
ycx_status launch_g(const GArgs& a, int g, unsigned nwg, hipStream_t st) {
  switch (g) {
    case 1: hipLaunchKernelGGL((gconv_kernel<T, K, 1>), dim3(nwg), dim3(256), 0, st, a); break;
    case 2: hipLaunchKernelGGL((gconv_kernel<T, K, 2>), dim3(nwg), dim3(256), 0, st, a); break;
    case 4: hipLaunchKernelGGL((gconv_kernel<T, K, 4>), dim3(nwg), dim3(256), 0, st, a); break;
    case 8: hipLaunchKernelGGL((gconv_kernel<T, K, 8>), dim3(nwg), dim3(256), 0, st, a); break;
    case 16: hipLaunchKernelGGL((gconv_kernel<T, K, 16>), dim3(nwg), dim3(256), 0, st, a); break;
    default: return YCX_ERR_UNSUPPORTED;
  }
  return ycx_launch_status();
}

template <typename T>
ycx_status launch_k(const GArgs& a, int k, int g, unsigned nwg, hipStream_t st) {
  switch (k) {
    case 3: return launch_g<T, 3>(a, g, nwg, st);
    case 5: return launch_g<T, 5>(a, g, nwg, st);
    case 7: return launch_g<T, 7>(a, g, nwg, st);
    case 11:  // depthwise only (validated by the caller)
      hipLaunchKernelGGL((gconv_kernel<T, 11, 1>), dim3(nwg), dim3(256), 0, st, a);
      return ycx_launch_status();
    default: return YCX_ERR_UNSUPPORTED;
  }
}

}  // namespace

extern "C" ycx_status ycx_conv2d_grouped(const ycx_conv_desc* d, const void* x, const float* w, const float* bias,
                                         void* y, const void* residual, void* stream) {
  YCX_CHECK_ARG(d);  // the descriptor is judged before the data pointers (checked below, before the launch)
  YCX_CHECK_ARG(d->n > 0 && d->h > 0 && d->w > 0 && d->cin > 0 && d->cout > 0 && d->ho > 0 && d->wo > 0);
  YCX_CHECK_ARG(d->kh > 0 && d->kw > 0 && d->stride > 0 && d->pad >= 0 && d->groups > 0);
  YCX_CHECK_ARG(d->cin % d->groups == 0 && d->cout % d->groups == 0);
  YCX_CHECK_ARG(d->in_c_off >= 0 && d->in_c_off + d->cin <= d->in_c_stride);
  YCX_CHECK_ARG(d->out_c_off >= 0 && d->out_c_off + d->cout <= d->out_c_stride);
  YCX_CHECK_ARG(d->ho == (d->h + 2 * d->pad - d->kh) / d->stride + 1);
  YCX_CHECK_ARG(d->wo == (d->w + 2 * d->pad - d->kw) / d->stride + 1);
  YCX_CHECK_ARG(!residual || (d->res_c_off >= 0 && d->res_c_off + d->cout <= d->res_c_stride));
  const int g = d->cin / d->groups;
  YCX_CHECK_SUPPORTED(d->groups > 1 && g == d->cout / d->groups && (g == 1 || g == 2 || g == 4 || g == 8 || g == 16));
  YCX_CHECK_SUPPORTED(d->kh == d->kw && (d->kh == 3 || d->kh == 5 || d->kh == 7 || (g == 1 && d->kh == 11)) &&
                      d->pad == d->kh / 2);
  YCX_CHECK_SUPPORTED(d->stride == 1 || d->stride == 2 || (g == 1 && (d->stride == 4 || d->stride == 8)));
  YCX_CHECK_SUPPORTED(d->dtype == YCX_DT_BF16 || d->dtype == YCX_DT_F16 || d->dtype == YCX_DT_F32);
  YCX_CHECK_SUPPORTED(d->act == YCX_ACT_NONE || d->act == YCX_ACT_SILU || d->act == YCX_ACT_LEAKY);
  YCX_CHECK_SUPPORTED(d->out_layout == YCX_OUT_NHWC && !d->in_pool && d->k_split <= 1);
  // a lane owns 8 channels: 16-byte vectors of 16-bit data (two of fp32) on both sides
  YCX_CHECK_SUPPORTED(d->cout % 8 == 0 && d->in_c_off % 8 == 0 && d->in_c_stride % 8 == 0 && d->out_c_off % 8 == 0 &&
                      d->out_c_stride % 8 == 0);
  if (residual) YCX_CHECK_SUPPORTED(d->res_c_off % 8 == 0 && d->res_c_stride % 8 == 0);
  YCX_CHECK_SUPPORTED((long long)d->n * d->h * d->w < (1LL << 31) && (long long)d->n * d->ho * d->wo < (1LL << 31));
  YCX_CHECK_ARG(x && w && bias && y);

  const int k = d->kh, s = d->stride, esz = d->dtype == YCX_DT_F32 ? 4 : 2;
  // Among the tiles whose input patch fits the LDS budget, the one that spends the fewest
  // pixel slots on this map (a workgroup runs its 64 pixel lanes once per 64 tile pixels);
  // ties go to the larger tile (less halo).
  static const int tiles[8][2] = {{16, 4}, {8, 4}, {16, 3}, {8, 3}, {4, 4}, {4, 3}, {2, 3}, {1, 3}};  // th, log2(tw)
  // strides 4 and 8 (depthwise): the patch grows with s, so smaller tiles (file header)
  static const int wide[8][2] = {{8, 2}, {4, 3}, {4, 2}, {4, 1}, {2, 2}, {2, 1}, {1, 1}, {1, 0}};
  int th = 0, twl = 0, ih = 0, iw = 0;
  long long best = -1;
  for (const auto& t : s > 2 ? wide : tiles) {
    const int tih = (t[0] - 1) * s + k, tiw = ((1 << t[1]) - 1) * s + k;
    if ((long long)tih * tiw * kChunk * esz > kXBytes) continue;
    const long long ntile = (long long)((d->ho + t[0] - 1) / t[0]) * ((d->wo + (1 << t[1]) - 1) >> t[1]);
    const long long cost = ntile * (((t[0] << t[1]) + 63) / 64);
    if (best < 0 || cost < best) {
      best = cost;
      th = t[0];
      twl = t[1];
      ih = tih;
      iw = tiw;
    }
  }
  YCX_CHECK_SUPPORTED(th > 0);
  GArgs a;
  a.x = x; a.w = w; a.bias = bias; a.y = y; a.res = residual;
  a.N = d->n; a.H = d->h; a.W = d->w; a.C = d->cin; a.in_coff = d->in_c_off; a.in_cs = d->in_c_stride;
  a.Ho = d->ho; a.Wo = d->wo; a.out_coff = d->out_c_off; a.out_cs = d->out_c_stride;
  a.res_coff = d->res_c_off; a.res_cs = d->res_c_stride;
  a.S = s; a.P = d->pad; a.act = d->act; a.slope = d->leaky_slope;
  a.th = th; a.tw_log2 = twl; a.ih = ih; a.iw = iw;
  a.tiles_x = (d->wo + (1 << twl) - 1) >> twl;
  a.tiles_y = (d->ho + th - 1) / th;
  a.n_chunks = (d->cin + kChunk - 1) / kChunk;
  a.wrows = k * k * kChunk * g <= kWFloats ? k : 1;
  YCX_CHECK_SUPPORTED(a.wrows * k * kChunk * g <= kWFloats);
  const long long nwg = (long long)d->n * a.tiles_y * a.tiles_x * a.n_chunks;
  YCX_CHECK_SUPPORTED(nwg < (1LL << 31));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  switch (d->dtype) {
    case YCX_DT_BF16: return launch_k<__bf16>(a, k, g, (unsigned)nwg, st);
    case YCX_DT_F16: return launch_k<_Float16>(a, k, g, (unsigned)nwg, st);
    default: return launch_k<float>(a, k, g, (unsigned)nwg, st);
  }
}
