// libycx_hip.so — the Classify head (ycx_classify): AdaptiveAvgPool2d(1), the centre tap of its Conv2d on
// the 1 x 1 map that leaves, Flatten (nets/common.py:815-825):
//   y[n, o] = bias[o] + sum_c w[o, c] * mean_hw x[n, :, :, c]
//
// Two launches on one stream. classify_pool reads the NHWC channel slice once (the layer's HBM traffic) and
// leaves the fp32 means in the workspace; classify_linear reads those [n][c] means and the fp32 weights.
// Every sum has a fixed order (per-lane ascending pixels, ascending pixel phases through LDS, a fixed
// xor-butterfly over the lanes) and nothing is added atomically, so a launch repeats bit for bit.
#include "ycx_internal.h"

namespace {

constexpr int kThreads = 256;
// The pool's blocks per launch below which a block takes fewer channel vectors and more pixel phases (down
// to 8 vectors, a 128-byte run per pixel): a constant of the kernel, not a property of the machine.
constexpr int kPoolBlocks = 512;
constexpr int kImgTile = 8;  // images per wave of the linear step

struct PoolArgs {
  const void* x;
  float* ws;
  int hw, c;
  int cv;            // vectors per pixel slice
  int cl_log2;       // log2(CL): channel vectors per block
  int ncb;           // blocks per image: ceil(cv / CL)
  long long in_off, in_stride;  // channel offset / pixel stride, in vectors
  float dequant;     // e4m3: 1 / s_in
  float hw_f;        // h * w, the mean's IEEE divisor
};

// One vector of VE consecutive channels as fp32. V: uint4 (16 bytes) or uint2 (8 bytes, e4m3 only).
template <int DT, typename V>
struct Unpack;
template <>
struct Unpack<YCX_DT_BF16, uint4> {
  static constexpr int VE = 8;
  static __device__ __forceinline__ void run(uint4 v, float* f) {
    const unsigned u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f[2 * j] = __uint_as_float(u[j] << 16);
      f[2 * j + 1] = __uint_as_float(u[j] & 0xffff0000u);
    }
  }
};
template <>
struct Unpack<YCX_DT_F16, uint4> {
  static constexpr int VE = 8;
  static __device__ __forceinline__ void run(uint4 v, float* f) {
    typedef __attribute__((ext_vector_type(2))) _Float16 h2;
    const unsigned u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const h2 p = __builtin_bit_cast(h2, u[j]);
      f[2 * j] = (float)p[0];
      f[2 * j + 1] = (float)p[1];
    }
  }
};
template <>
struct Unpack<YCX_DT_F32, uint4> {
  static constexpr int VE = 4;
  static __device__ __forceinline__ void run(uint4 v, float* f) {
    f[0] = __uint_as_float(v.x); f[1] = __uint_as_float(v.y);
    f[2] = __uint_as_float(v.z); f[3] = __uint_as_float(v.w);
  }
};
__device__ __forceinline__ void f8x4(unsigned u, float* f) {
  f[0] = __builtin_amdgcn_cvt_f32_fp8((int)u, 0); f[1] = __builtin_amdgcn_cvt_f32_fp8((int)u, 1);
  f[2] = __builtin_amdgcn_cvt_f32_fp8((int)u, 2); f[3] = __builtin_amdgcn_cvt_f32_fp8((int)u, 3);
}
template <>
struct Unpack<YCX_DT_FP8, uint4> {
  static constexpr int VE = 16;
  static __device__ __forceinline__ void run(uint4 v, float* f) {
    f8x4(v.x, f); f8x4(v.y, f + 4); f8x4(v.z, f + 8); f8x4(v.w, f + 12);
  }
};
template <>
struct Unpack<YCX_DT_FP8, uint2> {
  static constexpr int VE = 8;
  static __device__ __forceinline__ void run(uint2 v, float* f) {
    f8x4(v.x, f); f8x4(v.y, f + 4);
  }
};

// Block b: image b / ncb, channel vectors [cb * CL, cb * CL + CL). Thread t: vector cl = t % CL of those,
// pixel phase pg = t / CL of PG = 256 / CL: it sums pixels pg, pg + PG, ... in that order. The phases of
// one channel are then summed in ascending order from LDS (sm[j][t]: component j of thread t, so both the
// stores and the reads of consecutive lanes fall on consecutive banks).
template <int DT, typename V>
__global__ void __launch_bounds__(kThreads) classify_pool(PoolArgs a) {
  typedef Unpack<DT, V> U;
  constexpr int VE = U::VE;
  __shared__ float sm[VE][kThreads];
  const int t = threadIdx.x;
  const int CL = 1 << a.cl_log2, PG = kThreads >> a.cl_log2;
  const int img = blockIdx.x / a.ncb, cb = blockIdx.x - img * a.ncb;
  const int cl = t & (CL - 1), pg = t >> a.cl_log2;
  const int vec = cb * CL + cl;
  float acc[VE];
#pragma unroll
  for (int j = 0; j < VE; ++j) acc[j] = 0.0f;
  if (vec < a.cv) {
    const V* __restrict__ px = reinterpret_cast<const V*>(a.x) + (long long)img * a.hw * a.in_stride + a.in_off + vec;
    int p = pg;
    for (; p + 3 * PG < a.hw; p += 4 * PG) {  // four loads in flight, added in pixel order
      V v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = px[(long long)(p + u * PG) * a.in_stride];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float f[VE];
        U::run(v[u], f);
#pragma unroll
        for (int j = 0; j < VE; ++j) acc[j] += f[j];
      }
    }
    for (; p < a.hw; p += PG) {
      float f[VE];
      U::run(px[(long long)p * a.in_stride], f);
#pragma unroll
      for (int j = 0; j < VE; ++j) acc[j] += f[j];
    }
  }
#pragma unroll
  for (int j = 0; j < VE; ++j) sm[j][t] = acc[j];
  __syncthreads();
  // CL * VE channels per block, one per thread and round
  for (int e = t; e < (VE << a.cl_log2); e += kThreads) {
    const int j = e >> a.cl_log2, l = e & (CL - 1);
    const int v2 = cb * CL + l;
    if (v2 >= a.cv) continue;
    float s = sm[j][l];
    for (int g = 1; g < PG; ++g) s += sm[j][(g << a.cl_log2) + l];
    if (DT == YCX_DT_FP8) s *= a.dequant;
    a.ws[(long long)img * a.c + v2 * VE + j] = s / a.hw_f;
  }
}

// Wave (blockIdx.x * 4 + wave) = output o; blockIdx.y = a tile of kImgTile images. Lanes run over c in
// float4 steps (c % 8 == 0); each weight vector meets the tile's means, which the other outputs' waves
// read too (L1 / L2). Then a fixed butterfly over the 64 lanes; lane 0 adds the bias and stores.
__global__ void __launch_bounds__(kThreads) classify_linear(const float* __restrict__ ws, const float* __restrict__ w,
                                                            const float* __restrict__ bias, float* __restrict__ y,
                                                            int n, int c, int cout) {
  const int lane = threadIdx.x & 63;
  const int o = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (o >= cout) return;  // wave-uniform
  const int n0 = blockIdx.y * kImgTile;
  const int ni = min(kImgTile, n - n0);
  float acc[kImgTile];
#pragma unroll
  for (int i = 0; i < kImgTile; ++i) acc[i] = 0.0f;
  const float4* __restrict__ wr = reinterpret_cast<const float4*>(w + (long long)o * c);
  const int c4 = c >> 2;
  for (int k = lane; k < c4; k += 64) {
    const float4 wv = wr[k];
#pragma unroll
    for (int i = 0; i < kImgTile; ++i) {
      if (i < ni) {
        const float4 m = reinterpret_cast<const float4*>(ws + (long long)(n0 + i) * c)[k];
        float s = acc[i];
        s = __builtin_fmaf(wv.x, m.x, s);
        s = __builtin_fmaf(wv.y, m.y, s);
        s = __builtin_fmaf(wv.z, m.z, s);
        s = __builtin_fmaf(wv.w, m.w, s);
        acc[i] = s;
      }
    }
  }
  const float b = bias ? bias[o] : 0.0f;
#pragma unroll
  for (int i = 0; i < kImgTile; ++i) {
    float s = acc[i];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if (lane == 0 && i < ni) y[(long long)(n0 + i) * cout + o] = s + b;
  }
}

template <int DT, typename V>
void pool_launch(const PoolArgs& a, long long blocks, hipStream_t st) {
  hipLaunchKernelGGL((classify_pool<DT, V>), dim3((unsigned)blocks), dim3(kThreads), 0, st, a);
}

}  // namespace

extern "C" ycx_status ycx_classify(const ycx_classify_desc* d, const void* x, const float* w, const float* bias,
                                   float* y, float* workspace, void* stream) {
  YCX_CHECK_ARG(d && x && w && y && workspace);
  YCX_CHECK_ARG(d->dtype == YCX_DT_BF16 || d->dtype == YCX_DT_F16 || d->dtype == YCX_DT_F32 ||
                d->dtype == YCX_DT_FP8);
  YCX_CHECK_ARG(d->n > 0 && d->h > 0 && d->w > 0 && d->c > 0 && d->cout > 0 && d->in_c_stride > 0);
  YCX_CHECK_ARG(d->c % 8 == 0 && d->in_c_off % 8 == 0 && d->in_c_stride % 8 == 0);
  YCX_CHECK_ARG(d->in_c_off >= 0 && (long long)d->in_c_off + d->c <= d->in_c_stride);
  const long long hw = (long long)d->h * d->w;
  YCX_CHECK_SUPPORTED(hw < (1LL << 24));  // h * w as an exact fp32 divisor, pixel indices in int

  // elements per vector: 16 bytes, or 8 for an e4m3 slice on 8- but not 16-channel bounds
  const bool f8 = d->dtype == YCX_DT_FP8;
  const bool v16 = !f8 || (d->c % 16 == 0 && d->in_c_off % 16 == 0 && d->in_c_stride % 16 == 0);
  const int ve = d->dtype == YCX_DT_F32 ? 4 : f8 ? (v16 ? 16 : 8) : 8;
  PoolArgs a;
  a.x = x; a.ws = workspace;
  a.hw = (int)hw; a.c = d->c;
  a.cv = d->c / ve;
  a.in_off = d->in_c_off / ve; a.in_stride = d->in_c_stride / ve;
  a.dequant = f8 ? d->dequant : 1.0f;
  a.hw_f = (float)hw;
  // CL: 64 vectors per block; halved while half a block still covers the slice, and, down to 8, while the
  // launch has fewer than kPoolBlocks blocks (more pixel phases per channel instead)
  int cl_log2 = 6;
  while (cl_log2 > 0 && (1 << (cl_log2 - 1)) >= a.cv) --cl_log2;
  while (cl_log2 > 3 && (long long)d->n * ycx_cdiv(a.cv, 1 << cl_log2) < kPoolBlocks) --cl_log2;
  a.cl_log2 = cl_log2;
  a.ncb = (int)ycx_cdiv(a.cv, 1 << cl_log2);
  const long long blocks = (long long)d->n * a.ncb;
  const unsigned lin_x = ycx_cdiv(d->cout, kThreads / 64), lin_y = ycx_cdiv(d->n, kImgTile);
  YCX_CHECK_SUPPORTED(blocks <= 0x7fffffffLL && lin_y <= 65535u);

  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  switch (d->dtype) {
    case YCX_DT_BF16: pool_launch<YCX_DT_BF16, uint4>(a, blocks, st); break;
    case YCX_DT_F16: pool_launch<YCX_DT_F16, uint4>(a, blocks, st); break;
    case YCX_DT_F32: pool_launch<YCX_DT_F32, uint4>(a, blocks, st); break;
    default:
      if (v16) pool_launch<YCX_DT_FP8, uint4>(a, blocks, st);
      else pool_launch<YCX_DT_FP8, uint2>(a, blocks, st);
  }
  if (hipGetLastError() != hipSuccess) return YCX_ERR_LAUNCH;
  hipLaunchKernelGGL(classify_linear, dim3(lin_x, lin_y), dim3(kThreads), 0, st, workspace, w, bias, y, d->n, d->c,
                     d->cout);
  return ycx_launch_status();
}
