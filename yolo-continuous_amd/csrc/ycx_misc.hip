// Data-movement kernels of the YOLO layer graph (NHWC, HBM-bound):
//   max-pool  : MP (k2 s2), SP (k s1 pad k//2), SPPCSPC pools (nets/common.py:25-40, 257)
//   copy      : Concat fallback when a producer cannot write its slice directly,
//               and nn.Upsample(None, 2, 'nearest') (cfg/net/yolov7.yaml:71,85)
// plus the static-plan executor (ycx_run_ops) that replaces the Python layer
// loop of Model.forward (nets/yolo.py:143-153), and its HIP-graph capture.
//
// Each thread moves one 16-byte vector (8 bf16 or 4 fp32 channels); consecutive
// threads take consecutive channel chunks of one pixel, so every wave reads and
// writes whole contiguous channel rows.
#include <dlfcn.h>
#include <stdio.h>
#include <vector>

#include "ycx_internal.h"

namespace {

template <typename T>
struct Vec;
template <>
struct Vec<__bf16> {
  typedef bf16x8 type;
  static constexpr int N = 8;
};
template <>
struct Vec<_Float16> {
  typedef __attribute__((ext_vector_type(8))) _Float16 type;
  static constexpr int N = 8;
};
template <>
struct Vec<float> {
  typedef f32x4 type;
  static constexpr int N = 4;
};

template <typename T>
__global__ void __launch_bounds__(256) maxpool_kernel(ycx_pool_desc d, const T* __restrict__ x,
                                                      T* __restrict__ y) {
  typedef typename Vec<T>::type V;
  constexpr int VN = Vec<T>::N;
  const int cv = d.c / VN;
  const long long total = (long long)d.n * d.ho * d.wo * cv;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    int c = (int)(i % cv);
    long long p = i / cv;
    int ox = (int)(p % d.wo);
    long long t = p / d.wo;
    int oy = (int)(t % d.ho);
    int n = (int)(t / d.ho);
    float m[VN];
#pragma unroll
    for (int j = 0; j < VN; ++j) m[j] = -INFINITY;
    const int y0 = oy * d.stride - d.pad, x0 = ox * d.stride - d.pad;
    const int ya = max(y0, 0), yb = min(y0 + d.k, d.h), xa = max(x0, 0), xb = min(x0 + d.k, d.w);
    for (int iy = ya; iy < yb; ++iy)
      for (int ix = xa; ix < xb; ++ix) {
        V v = *reinterpret_cast<const V*>(x + (((size_t)n * d.h + iy) * d.w + ix) * d.in_c_stride +
                                          d.in_c_off + c * VN);
#pragma unroll
        for (int j = 0; j < VN; ++j) m[j] = ycx_pool_max(m[j], (float)v[j]);
      }
    V o;
#pragma unroll
    for (int j = 0; j < VN; ++j) o[j] = (T)m[j];
    *reinterpret_cast<V*>(y + (((size_t)n * d.ho + oy) * d.wo + ox) * d.out_c_stride + d.out_c_off +
                          c * VN) = o;
  }
}

// The same pool on a 2-D grid: blockIdx.y = output row (n * ho + oy), x over (ox, channel
// chunk) -- 32-bit index math (the flat kernel's 64-bit div/mod chain was a VALU cost on the
// HBM-bound k2s2 pools).
template <typename T>
__global__ void __launch_bounds__(256) maxpool_rows_kernel(ycx_pool_desc d, const T* __restrict__ x,
                                                           T* __restrict__ y) {
  typedef typename Vec<T>::type V;
  constexpr int VN = Vec<T>::N;
  const int cv = d.c / VN;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= d.wo * cv) return;
  const int row = blockIdx.y, n = row / d.ho, oy = row - n * d.ho;
  const int ox = i / cv, c = i - ox * cv;
  float m[VN];
#pragma unroll
  for (int j = 0; j < VN; ++j) m[j] = -INFINITY;
  const int y0 = oy * d.stride - d.pad, x0 = ox * d.stride - d.pad;
  const int ya = max(y0, 0), yb = min(y0 + d.k, d.h), xa = max(x0, 0), xb = min(x0 + d.k, d.w);
  for (int iy = ya; iy < yb; ++iy) {
    const T* rowp = x + ((size_t)(n * d.h + iy) * d.w) * d.in_c_stride + d.in_c_off + c * VN;
    for (int ix = xa; ix < xb; ++ix) {
      const V v = *reinterpret_cast<const V*>(rowp + (size_t)ix * d.in_c_stride);
#pragma unroll
      for (int j = 0; j < VN; ++j) m[j] = ycx_pool_max(m[j], (float)v[j]);
    }
  }
  V o;
#pragma unroll
  for (int j = 0; j < VN; ++j) o[j] = (T)m[j];
  *reinterpret_cast<V*>(y + ((size_t)row * d.wo + ox) * d.out_c_stride + d.out_c_off + c * VN) = o;
}

template <typename T>
__global__ void __launch_bounds__(256) copy_kernel(ycx_copy_desc d, const T* __restrict__ x,
                                                   T* __restrict__ y) {
  typedef typename Vec<T>::type V;
  constexpr int VN = Vec<T>::N;
  const int cv = d.c / VN;
  const int ho = d.h * d.scale, wo = d.w * d.scale;
  const long long total = (long long)d.n * ho * wo * cv;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    int c = (int)(i % cv);
    long long p = i / cv;
    int ox = (int)(p % wo);
    long long t = p / wo;
    int oy = (int)(t % ho);
    int n = (int)(t / ho);
    int iy = oy / d.scale, ix = ox / d.scale;  // nearest: floor(out * in/out)
    V v = *reinterpret_cast<const V*>(x + (((size_t)n * d.h + iy) * d.w + ix) * d.in_c_stride +
                                      d.in_c_off + c * VN);
    if (d.out_layout == YCX_OUT_NCHW_F32) {
      float* yf = reinterpret_cast<float*>(y);
#pragma unroll
      for (int j = 0; j < VN; ++j)
        yf[(((size_t)n * d.out_c_stride + d.out_c_off + c * VN + j) * ho + oy) * wo + ox] = (float)v[j];
    } else {
      *reinterpret_cast<V*>(y + (((size_t)n * ho + oy) * wo + ox) * d.out_c_stride + d.out_c_off + c * VN) = v;
    }
  }
}

// ---- fp8 (OCP e4m3fn) variants: 8 channels = 8 bytes per thread ----
__device__ __forceinline__ void f8x8_unpack(uint2 v, float f[8]) {
  f[0] = __builtin_amdgcn_cvt_f32_fp8((int)v.x, 0); f[1] = __builtin_amdgcn_cvt_f32_fp8((int)v.x, 1);
  f[2] = __builtin_amdgcn_cvt_f32_fp8((int)v.x, 2); f[3] = __builtin_amdgcn_cvt_f32_fp8((int)v.x, 3);
  f[4] = __builtin_amdgcn_cvt_f32_fp8((int)v.y, 0); f[5] = __builtin_amdgcn_cvt_f32_fp8((int)v.y, 1);
  f[6] = __builtin_amdgcn_cvt_f32_fp8((int)v.y, 2); f[7] = __builtin_amdgcn_cvt_f32_fp8((int)v.y, 3);
}
__device__ __forceinline__ uint32_t f8x4_pack_sat(float a, float b, float c, float d) {
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(fminf(fmaxf(a, -448.f), 448.f), fminf(fmaxf(b, -448.f), 448.f), 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(fminf(fmaxf(c, -448.f), 448.f), fminf(fmaxf(d, -448.f), 448.f), w, true);
  return (uint32_t)w;
}

// Max over the window in fp32 of the decoded bytes; the max is one of the
// inputs, so re-encoding it is exact (input and output share the scale).
__global__ void __launch_bounds__(256) maxpool_f8_kernel(ycx_pool_desc d, const uint8_t* __restrict__ x,
                                                         uint8_t* __restrict__ y) {
  const int cv = d.c / 8;
  const long long total = (long long)d.n * d.ho * d.wo * cv;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    int c = (int)(i % cv);
    long long p = i / cv;
    int ox = (int)(p % d.wo);
    long long t = p / d.wo;
    int oy = (int)(t % d.ho);
    int n = (int)(t / d.ho);
    float m[8], f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) m[j] = -INFINITY;
    const int y0 = oy * d.stride - d.pad, x0 = ox * d.stride - d.pad;
    const int ya = max(y0, 0), yb = min(y0 + d.k, d.h), xa = max(x0, 0), xb = min(x0 + d.k, d.w);
    for (int iy = ya; iy < yb; ++iy)
      for (int ix = xa; ix < xb; ++ix) {
        f8x8_unpack(*reinterpret_cast<const uint2*>(x + (((size_t)n * d.h + iy) * d.w + ix) * d.in_c_stride +
                                                    d.in_c_off + c * 8), f);
#pragma unroll
        for (int j = 0; j < 8; ++j) m[j] = fmaxf(m[j], f[j]);
      }
    *reinterpret_cast<uint2*>(y + (((size_t)n * d.ho + oy) * d.wo + ox) * d.out_c_stride + d.out_c_off + c * 8) =
        make_uint2(f8x4_pack_sat(m[0], m[1], m[2], m[3]), f8x4_pack_sat(m[4], m[5], m[6], m[7]));
  }
}

// Byte copy (same scale on both sides), or decode to fp32 NCHW x dequant.
__global__ void __launch_bounds__(256) copy_f8_kernel(ycx_copy_desc d, const uint8_t* __restrict__ x,
                                                      uint8_t* __restrict__ y) {
  const int cv = d.c / 8;
  const int ho = d.h * d.scale, wo = d.w * d.scale;
  const long long total = (long long)d.n * ho * wo * cv;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    int c = (int)(i % cv);
    long long p = i / cv;
    int ox = (int)(p % wo);
    long long t = p / wo;
    int oy = (int)(t % ho);
    int n = (int)(t / ho);
    int iy = oy / d.scale, ix = ox / d.scale;
    const uint2 v = *reinterpret_cast<const uint2*>(x + (((size_t)n * d.h + iy) * d.w + ix) * d.in_c_stride +
                                                    d.in_c_off + c * 8);
    if (d.out_layout == YCX_OUT_NCHW_F32) {
      float f[8];
      f8x8_unpack(v, f);
      float* yf = reinterpret_cast<float*>(y);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        yf[(((size_t)n * d.out_c_stride + d.out_c_off + c * 8 + j) * ho + oy) * wo + ox] = f[j] * d.dequant;
    } else {
      *reinterpret_cast<uint2*>(y + (((size_t)n * ho + oy) * wo + ox) * d.out_c_stride + d.out_c_off + c * 8) = v;
    }
  }
}

__global__ void __launch_bounds__(256) quantize_f8_kernel(const float* __restrict__ x, uint8_t* __restrict__ y,
                                                          long long n, float scale) {
  for (long long i = (blockIdx.x * (long long)blockDim.x + threadIdx.x) * 4; i < n;
       i += (long long)gridDim.x * blockDim.x * 4) {
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = i + j < n ? x[i + j] * scale : 0.0f;
    const uint32_t w = f8x4_pack_sat(v[0], v[1], v[2], v[3]);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (i + j < n) y[i + j] = (uint8_t)(w >> (8 * j));
  }
}

// Cascade of `levels` k x k 'same' max-pools (stride 1) in one launch: one workgroup per
// (image, CC-channel slice) holds the whole H x W plane in LDS (raw elements), and each level
// is a row pass then a column pass (a k x k max with -inf padding is separable); level i goes
// to channels out_c_off + i*c. E = bytes per element (2 bf16 / fp16 (HALF), 1 e4m3); 16-byte chunks.
// e4m3 activations hold no NaN (the fp8 stores saturate): the fp8 cascade keeps fmaxf
template <int E>
__device__ __forceinline__ float pool_max_e(float a, float b) {
  if constexpr (E == 1) return fmaxf(a, b);
  else return ycx_pool_max(a, b);
}
template <int E, bool HALF = false>
__device__ __forceinline__ void chunk_to_f(uint4 v, float (&f)[16 / E]) {
  if constexpr (E == 2 && HALF) {
    const _Float16* b = reinterpret_cast<const _Float16*>(&v);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = (float)b[j];
  } else if constexpr (E == 2) {
    const __bf16* b = reinterpret_cast<const __bf16*>(&v);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = (float)b[j];
  } else {
    float* g = f;
    f8x8_unpack(make_uint2(v.x, v.y), g);
    f8x8_unpack(make_uint2(v.z, v.w), g + 8);
  }
}
template <int E, bool HALF = false>
__device__ __forceinline__ uint4 f_to_chunk(const float (&f)[16 / E]) {
  uint4 v;
  if constexpr (E == 2 && HALF) {
    _Float16* b = reinterpret_cast<_Float16*>(&v);
#pragma unroll
    for (int j = 0; j < 8; ++j) b[j] = (_Float16)f[j];  // exact: every value is an input element
  } else if constexpr (E == 2) {
    __bf16* b = reinterpret_cast<__bf16*>(&v);
#pragma unroll
    for (int j = 0; j < 8; ++j) b[j] = (__bf16)f[j];  // exact: every value is an input element
  } else {
    v.x = f8x4_pack_sat(f[0], f[1], f[2], f[3]);
    v.y = f8x4_pack_sat(f[4], f[5], f[6], f[7]);
    v.z = f8x4_pack_sat(f[8], f[9], f[10], f[11]);
    v.w = f8x4_pack_sat(f[12], f[13], f[14], f[15]);
  }
  return v;
}

template <int E, bool HALF = false>
__global__ void __launch_bounds__(256) maxpool_cascade_kernel(ycx_pool_desc d, int cc, const uint8_t* __restrict__ x,
                                                              uint8_t* __restrict__ y) {
  extern __shared__ uint4 lds_chunks[];
  constexpr int NE = 16 / E;
  const int H = d.h, W = d.w, HW = H * W, r = d.k / 2;
  const int nchunk = cc * E / 16;  // 16-byte chunks per pixel in this slice
  const int items = HW * nchunk;
  const int n = blockIdx.x / (d.c / cc), c0 = (blockIdx.x % (d.c / cc)) * cc;
  uint4* S = lds_chunks;           // [HW][nchunk]: the level's source
  uint4* T = lds_chunks + items;   // [HW][nchunk]: after the row pass
  const size_t px0 = (size_t)n * HW;
  for (int i = threadIdx.x; i < items; i += blockDim.x) {
    const int pix = i / nchunk, g = i - pix * nchunk;
    S[i] = *reinterpret_cast<const uint4*>(x + ((px0 + pix) * d.in_c_stride + d.in_c_off + c0) * E + g * 16);
  }
  __syncthreads();
  for (int lv = 0; lv < d.levels; ++lv) {
    for (int i = threadIdx.x; i < items; i += blockDim.x) {  // row pass
      const int pix = i / nchunk, g = i - pix * nchunk, yy = pix / W, xx = pix - yy * W;
      float m[NE], f[NE];
#pragma unroll
      for (int j = 0; j < NE; ++j) m[j] = -INFINITY;
      for (int xi = max(xx - r, 0); xi <= min(xx + r, W - 1); ++xi) {
        chunk_to_f<E, HALF>(S[(yy * W + xi) * nchunk + g], f);
#pragma unroll
        for (int j = 0; j < NE; ++j) m[j] = pool_max_e<E>(m[j], f[j]);
      }
      T[i] = f_to_chunk<E, HALF>(m);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < items; i += blockDim.x) {  // column pass: the level's output
      const int pix = i / nchunk, g = i - pix * nchunk, yy = pix / W, xx = pix - yy * W;
      float m[NE], f[NE];
#pragma unroll
      for (int j = 0; j < NE; ++j) m[j] = -INFINITY;
      for (int yi = max(yy - r, 0); yi <= min(yy + r, H - 1); ++yi) {
        chunk_to_f<E, HALF>(T[(yi * W + xx) * nchunk + g], f);
#pragma unroll
        for (int j = 0; j < NE; ++j) m[j] = pool_max_e<E>(m[j], f[j]);
      }
      const uint4 v = f_to_chunk<E, HALF>(m);
      S[i] = v;  // the next level's source (every row pass read of S is behind the barrier above)
      *reinterpret_cast<uint4*>(y + ((px0 + pix) * d.out_c_stride + d.out_c_off + lv * d.c + c0) * E + g * 16) = v;
    }
    __syncthreads();
  }
}

unsigned grid_for(long long total) {
  long long b = (total + 255) / 256;
  if (b > 256LL * 16) b = 256LL * 16;  // grid-stride beyond 16 blocks per CU
  return (unsigned)(b < 1 ? 1 : b);
}

}  // namespace

extern "C" ycx_status ycx_maxpool(const ycx_pool_desc* d, const void* x, void* y, void* stream) {
  YCX_CHECK_ARG(d && x && y);
  YCX_CHECK_ARG(d->n > 0 && d->h > 0 && d->w > 0 && d->c > 0 && d->k > 0 && d->stride > 0 && d->pad >= 0);
  YCX_CHECK_ARG(d->ho == (d->h + 2 * d->pad - d->k) / d->stride + 1);
  YCX_CHECK_ARG(d->wo == (d->w + 2 * d->pad - d->k) / d->stride + 1);
  YCX_CHECK_ARG(d->pad * 2 <= d->k);  // torch: pad <= k/2
  YCX_CHECK_ARG(d->in_c_off + d->c <= d->in_c_stride && d->out_c_off + d->c <= d->out_c_stride);
  YCX_CHECK_SUPPORTED(d->dtype == YCX_DT_BF16 || d->dtype == YCX_DT_F32 || d->dtype == YCX_DT_FP8 ||
                      d->dtype == YCX_DT_F16);
  const int vn = d->dtype == YCX_DT_F32 ? 4 : 8;
  YCX_CHECK_SUPPORTED(d->c % vn == 0 && d->in_c_off % vn == 0 && d->in_c_stride % vn == 0 &&
                      d->out_c_off % vn == 0 && d->out_c_stride % vn == 0);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bool h16 = d->dtype == YCX_DT_F16;
  if (d->levels > 1) {
    YCX_CHECK_ARG(d->stride == 1 && d->k % 2 == 1 && d->pad == d->k / 2 && d->ho == d->h && d->wo == d->w);
    YCX_CHECK_ARG(d->out_c_off + d->levels * d->c <= d->out_c_stride);
    YCX_CHECK_SUPPORTED(d->dtype == YCX_DT_BF16 || d->dtype == YCX_DT_FP8 || h16);
    const int esz = d->dtype == YCX_DT_FP8 ? 1 : 2;
    // widest channel slice (16-byte multiple, dividing c) whose two planes fit 64 KB of LDS
    const long long hw = (long long)d->h * d->w;
    int cc = 0;
    for (int t = 128; t * esz >= 16; t >>= 1)
      if (d->c % t == 0 && 2 * hw * t * esz <= 65536) { cc = t; break; }
    YCX_CHECK_SUPPORTED(cc > 0);
    const dim3 g((unsigned)(d->n * (d->c / cc)));
    const size_t lds = (size_t)(2 * hw * cc * esz);
    if (h16)
      hipLaunchKernelGGL((maxpool_cascade_kernel<2, true>), g, dim3(256), lds, st, *d, cc, (const uint8_t*)x,
                         (uint8_t*)y);
    else if (esz == 2)
      hipLaunchKernelGGL(maxpool_cascade_kernel<2>, g, dim3(256), lds, st, *d, cc, (const uint8_t*)x, (uint8_t*)y);
    else
      hipLaunchKernelGGL(maxpool_cascade_kernel<1>, g, dim3(256), lds, st, *d, cc, (const uint8_t*)x, (uint8_t*)y);
    return ycx_launch_status();
  }
  long long total = (long long)d->n * d->ho * d->wo * (d->c / vn);
  const long long rows = (long long)d->n * d->ho, rowlen = (long long)d->wo * (d->c / vn);
  if (d->dtype != YCX_DT_FP8 && rows <= 65535 && total < (1LL << 31) &&
      (long long)d->n * d->h * d->w * d->in_c_stride < (1LL << 31)) {
    const dim3 g((unsigned)((rowlen + 255) / 256), (unsigned)rows);
    if (h16)
      hipLaunchKernelGGL(maxpool_rows_kernel<_Float16>, g, dim3(256), 0, st, *d, (const _Float16*)x, (_Float16*)y);
    else if (d->dtype == YCX_DT_BF16)
      hipLaunchKernelGGL(maxpool_rows_kernel<__bf16>, g, dim3(256), 0, st, *d, (const __bf16*)x, (__bf16*)y);
    else
      hipLaunchKernelGGL(maxpool_rows_kernel<float>, g, dim3(256), 0, st, *d, (const float*)x, (float*)y);
    return ycx_launch_status();
  }
  if (d->dtype == YCX_DT_FP8)
    hipLaunchKernelGGL(maxpool_f8_kernel, dim3(grid_for(total)), dim3(256), 0, st, *d, (const uint8_t*)x,
                       (uint8_t*)y);
  else if (h16)
    hipLaunchKernelGGL(maxpool_kernel<_Float16>, dim3(grid_for(total)), dim3(256), 0, st, *d,
                       (const _Float16*)x, (_Float16*)y);
  else if (d->dtype == YCX_DT_BF16)
    hipLaunchKernelGGL(maxpool_kernel<__bf16>, dim3(grid_for(total)), dim3(256), 0, st, *d,
                       (const __bf16*)x, (__bf16*)y);
  else
    hipLaunchKernelGGL(maxpool_kernel<float>, dim3(grid_for(total)), dim3(256), 0, st, *d, (const float*)x,
                       (float*)y);
  return ycx_launch_status();
}

extern "C" ycx_status ycx_copy_channels(const ycx_copy_desc* d, const void* x, void* y, void* stream) {
  YCX_CHECK_ARG(d && x && y);
  YCX_CHECK_ARG(d->n > 0 && d->h > 0 && d->w > 0 && d->c > 0 && (d->scale == 1 || d->scale == 2));
  YCX_CHECK_ARG(d->in_c_off + d->c <= d->in_c_stride && d->out_c_off + d->c <= d->out_c_stride);
  YCX_CHECK_SUPPORTED(d->out_layout == YCX_OUT_NHWC || d->out_layout == YCX_OUT_NCHW_F32);
  YCX_CHECK_SUPPORTED(d->dtype == YCX_DT_BF16 || d->dtype == YCX_DT_F32 || d->dtype == YCX_DT_FP8 ||
                      d->dtype == YCX_DT_F16);
  const int vn = d->dtype == YCX_DT_F32 ? 4 : 8;
  YCX_CHECK_SUPPORTED(d->c % vn == 0 && d->in_c_off % vn == 0 && d->in_c_stride % vn == 0 &&
                      d->out_c_off % vn == 0 && d->out_c_stride % vn == 0);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  long long total = (long long)d->n * d->h * d->scale * d->w * d->scale * (d->c / vn);
  if (d->dtype == YCX_DT_FP8)
    hipLaunchKernelGGL(copy_f8_kernel, dim3(grid_for(total)), dim3(256), 0, st, *d, (const uint8_t*)x,
                       (uint8_t*)y);
  else if (d->dtype == YCX_DT_F16)
    hipLaunchKernelGGL(copy_kernel<_Float16>, dim3(grid_for(total)), dim3(256), 0, st, *d, (const _Float16*)x,
                       (_Float16*)y);
  else if (d->dtype == YCX_DT_BF16)
    hipLaunchKernelGGL(copy_kernel<__bf16>, dim3(grid_for(total)), dim3(256), 0, st, *d, (const __bf16*)x,
                       (__bf16*)y);
  else
    hipLaunchKernelGGL(copy_kernel<float>, dim3(grid_for(total)), dim3(256), 0, st, *d, (const float*)x,
                       (float*)y);
  return ycx_launch_status();
}

extern "C" ycx_status ycx_quantize_fp8(const float* x, void* y, int64_t n, float scale, void* stream) {
  YCX_CHECK_ARG(n >= 0 && (n == 0 || (x && y)));
  if (n == 0) return YCX_OK;
  hipLaunchKernelGGL(quantize_f8_kernel, dim3(grid_for((n + 3) / 4)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), x, (uint8_t*)y, (long long)n, scale);
  return ycx_launch_status();
}

// ---------------------------------------------------------------------------
// Static plan executor: Model.forward's interpreter loop (nets/yolo.py:145-151)
// becomes one native loop over pre-validated op descriptors.
// ---------------------------------------------------------------------------
// ycx_depth_desc joined the op's union without growing it (ycx.h: the ABI version and ycx_struct_size(8) stay)
static_assert(sizeof(ycx_depth_desc) <= sizeof(ycx_conv_desc[2]), "ycx_depth_desc must not grow ycx_op's union");
static_assert(sizeof(ycx_classify_desc) <= sizeof(ycx_conv_desc[2]), "ycx_classify_desc must not grow ycx_op's union");

static ycx_status run_one(const ycx_op& op, void* stream) {
  switch (op.kind) {
    case YCX_OP_CONV:
      return ycx_conv2d_ws(&op.d.conv, op.in, op.weight, op.bias, op.out, op.residual, op.workspace,
                           op.workspace ? ycx_conv_workspace_size(&op.d.conv) : 0, stream);
    case YCX_OP_STEM:
      return ycx_stem_conv(&op.d.conv, (const float*)op.in, (const float*)op.weight, op.bias, op.out, stream);
    case YCX_OP_STEM_REORG:
      return ycx_stem_conv_reorg(&op.d.conv, (const float*)op.in, (const float*)op.weight, op.bias, op.out, stream);
    case YCX_OP_GCONV:
      return ycx_conv2d_grouped(&op.d.conv, op.in, (const float*)op.weight, op.bias, op.out, op.residual,
                                stream);
    case YCX_OP_DECONV:
      return ycx_deconv2d(&op.d.conv, op.in, op.weight, op.bias, op.out, stream);
    case YCX_OP_GHOST:
      return ycx_ghost_dw(&op.d.conv, op.in, (const float*)op.weight, op.bias, op.out, op.residual, stream);
    case YCX_OP_POOL:
      return ycx_maxpool(&op.d.pool, op.in, op.out, stream);
    case YCX_OP_COPY:
      return ycx_copy_channels(&op.d.copy, op.in, op.out, stream);
    case YCX_OP_DEPTH:
      return ycx_space_depth(&op.d.depth, op.in, op.out, stream);
    case YCX_OP_CLASSIFY:
      return ycx_classify(&op.d.classify, op.in, (const float*)op.weight, op.bias, (float*)op.out,
                          (float*)op.workspace, stream);
    case YCX_OP_STEM2:
      return ycx_stem_conv2(&op.d.pair[0], &op.d.pair[1], (const float*)op.in, (const float*)op.weight, op.bias,
                            op.weight2, op.bias2, op.out, stream);
    case YCX_OP_CONV_PAIR:
      if (op.out3)
        return ycx_conv2d_pair_pool(&op.d.pair[0], &op.d.pair[1], &op.conv3, op.in, op.weight, op.bias, op.out,
                                    op.weight2, op.bias2, op.out2, op.weight3, op.bias3, op.out3, stream);
      return ycx_conv2d_pair(&op.d.pair[0], &op.d.pair[1], op.in, op.weight, op.bias, op.out, op.weight2, op.bias2,
                             op.out2, stream);
    case YCX_OP_HEAD:
      return ycx_conv2d_head(&op.d.head.conv, &op.d.head.head, op.in, op.weight, op.bias, (float*)op.out,
                             (ycx_cand*)op.cand, op.cand_rows, op.cand_counts, op.status, stream);
    default:
      return YCX_ERR_BAD_ARG;
  }
}

// roctx ranges per op (SURVEY §5 tracing): off unless ycx_set_trace(1). One range per
// op names its index, kind, kernel tile and shape, so a `rocprofv3 --marker-trace`
// timeline of an eager forward lines each kernel up with its Model.forward layer.
// (A HIP-graph replay has no host loop: trace an eager run.)
// The roctx library is resolved with dlopen on the first ycx_set_trace(1), so the product
// library carries no link-time dependency on the profiler SDK.
static int g_trace = 0;
static int (*g_roctx_push)(const char*) = nullptr;
static int (*g_roctx_pop)() = nullptr;

extern "C" ycx_status ycx_set_trace(int32_t on) {
  if (!on) {
    g_trace = 0;
    return YCX_OK;
  }
  if (!g_roctx_push) {
    void* h = dlopen("librocprofiler-sdk-roctx.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) return YCX_ERR_UNSUPPORTED;
    auto push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
    auto pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
    if (!push || !pop) return YCX_ERR_UNSUPPORTED;
    g_roctx_pop = pop;
    g_roctx_push = push;
  }
  g_trace = 1;
  return YCX_OK;
}

static void trace_push(int32_t i, const ycx_op& op) {
  static const char* kinds[] = {"?", "conv", "stem", "pool", "copy", "stem2", "head", "conv_pair", "stem_reorg",
                                "gconv", "deconv", "ghost", "depth", "classify"};
  const char* k = (op.kind >= 1 && op.kind <= 13) ? kinds[op.kind] : kinds[0];
  char buf[160];
  if (op.kind == YCX_OP_CONV || op.kind == YCX_OP_STEM || op.kind == YCX_OP_HEAD || op.kind == YCX_OP_STEM2 ||
      op.kind == YCX_OP_CONV_PAIR || op.kind == YCX_OP_STEM_REORG || op.kind == YCX_OP_GCONV || op.kind == YCX_OP_DECONV ||
      op.kind == YCX_OP_GHOST) {
    const ycx_conv_desc& c = op.kind == YCX_OP_HEAD ? op.d.head.conv
                             : op.kind == YCX_OP_STEM2 || op.kind == YCX_OP_CONV_PAIR ? op.d.pair[1] : op.d.conv;
    snprintf(buf, sizeof buf, "op%d %s %s n%d %dx%d %d->%d k%d s%d", i, k,
             op.kind == YCX_OP_CONV ? ycx_conv_tile_name(c.tile ? c.tile : ycx_conv_pick_tile(&c)) : "", c.n, c.h,
             c.w, c.cin, c.cout, c.kh, c.stride);
  } else {
    snprintf(buf, sizeof buf, "op%d %s", i, k);
  }
  g_roctx_push(buf);
}

extern "C" ycx_status ycx_run_ops(const ycx_op* ops, int32_t n_ops, void* stream, void* const* events) {
  YCX_CHECK_ARG(ops && n_ops >= 0);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  for (int32_t i = 0; i < n_ops; ++i) {
    if (events && hipEventRecord(reinterpret_cast<hipEvent_t>(events[i]), st) != hipSuccess)
      return YCX_ERR_LAUNCH;
    if (g_trace) trace_push(i, ops[i]);
    ycx_status s = run_one(ops[i], stream);
    if (g_trace) g_roctx_pop();
    if (s != YCX_OK) return s;
  }
  if (events && hipEventRecord(reinterpret_cast<hipEvent_t>(events[n_ops]), st) != hipSuccess)
    return YCX_ERR_LAUNCH;
  return YCX_OK;
}

extern "C" ycx_status ycx_graph_capture(const ycx_op* ops, int32_t n_ops, void* stream, void** graph_exec) {
  YCX_CHECK_ARG(ops && graph_exec && stream);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipGraph_t g = nullptr;
  if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess) return YCX_ERR_LAUNCH;
  ycx_status s = ycx_run_ops(ops, n_ops, stream, nullptr);
  hipError_t e = hipStreamEndCapture(st, &g);
  if (s != YCX_OK) {
    if (g) (void)hipGraphDestroy(g);
    return s;
  }
  if (e != hipSuccess || !g) return YCX_ERR_LAUNCH;
  hipGraphExec_t ex = nullptr;
  e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (e != hipSuccess) return YCX_ERR_LAUNCH;
  *graph_exec = ex;
  return YCX_OK;
}

extern "C" ycx_status ycx_graph_launch(void* graph_exec, void* stream) {
  YCX_CHECK_ARG(graph_exec);
  return hipGraphLaunch(reinterpret_cast<hipGraphExec_t>(graph_exec), reinterpret_cast<hipStream_t>(stream)) ==
                 hipSuccess
             ? YCX_OK
             : YCX_ERR_LAUNCH;
}

extern "C" ycx_status ycx_graph_destroy(void* graph_exec) {
  YCX_CHECK_ARG(graph_exec);
  return hipGraphExecDestroy(reinterpret_cast<hipGraphExec_t>(graph_exec)) == hipSuccess ? YCX_OK
                                                                                         : YCX_ERR_LAUNCH;
}

#ifdef YCX_DEBUG_BOUNDS
extern "C" ycx_status ycx_dbg_bounds_conv(unsigned*, int);
extern "C" ycx_status ycx_dbg_bounds_conv_f16(unsigned*, int);
#endif

extern "C" ycx_status ycx_debug_bounds(uint32_t* out, int32_t reset) {
  YCX_CHECK_ARG(out);
  out[0] = out[1] = 0;
#ifdef YCX_DEBUG_BOUNDS
  ycx_status s = ycx_dbg_bounds_conv(out, reset);
  if (s == YCX_OK) s = ycx_dbg_bounds_conv_f16(out, reset);
  return s;
#else
  (void)reset;
  return YCX_ERR_UNSUPPORTED;  // a release build: the store checks are compiled out
#endif
}

extern "C" int ycx_abi_version(void) { return YCX_ABI_VERSION; }

extern "C" size_t ycx_struct_size(int32_t which) {
  switch (which) {
    case 0: return sizeof(ycx_conv_desc);
    case 1: return sizeof(ycx_pool_desc);
    case 2: return sizeof(ycx_copy_desc);
    case 3: return sizeof(ycx_decode_desc);
    case 4: return sizeof(ycx_cand);
    case 5: return sizeof(ycx_filter_desc);
    case 6: return sizeof(ycx_decode_filter_desc);
    case 7: return sizeof(ycx_nms_desc);
    case 8: return sizeof(ycx_op);
    case 9: return sizeof(ycx_letterbox_desc);
    case 10: return sizeof(ycx_correct_desc);
    case 11: return sizeof(ycx_head_desc);
    default: return 0;
  }
}

extern "C" const char* ycx_strerror(ycx_status s) {
  switch (s) {
    case YCX_OK: return "ok";
    case YCX_ERR_BAD_ARG: return "ycx: bad argument (null pointer or inconsistent shape)";
    case YCX_ERR_UNSUPPORTED: return "ycx: unsupported shape/dtype for the HIP kernels";
    case YCX_ERR_LAUNCH: return "ycx: HIP launch/runtime failure";
    case YCX_ERR_CAPACITY: return "ycx: workspace or output capacity too small";
    default: return "ycx: unknown status";
  }
}
