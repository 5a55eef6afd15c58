// ycx_deconv2d: NHWC transposed convolution with kernel == stride == s in {2, 4, 8}, pad 0
// (nn.ConvTranspose2d as RobustConv2 uses it, nets/common.py:133-134; the learned x-s upsample).
//
//   y[n, oh, ow, co] = act(bias[co] + sum_ci x[n, oh / s, ow / s, ci] * W[ci, co, oh % s, ow % s])
//
// The s x s windows do not overlap, so the op is one GEMM whose result is scattered:
//   rows    R = s*s*cout  (tap-major: row = (dy*s + dx)*cout + co; the packed weights are [R][cin])
//   columns M = n*h*w     low-resolution pixels
//   K       = cin
// and element (row, m) lands at pixel (y*s + dy, x*s + dx) of image n, channel co. The output is
// s*s times the input, so the store is the floor; the [n][h][w][R] matrix never exists in memory.
//
// 16-bit (bf16 / fp16): v_mfma_f32_16x16x32, the weights as the A operand and the pixels as B, so a
// lane's four accumulator registers are four consecutive rows (output channels) of one pixel.
//   * a workgroup (4 waves, 2 x 2) owns 128 rows x 128 pixels; a wave 64 x 64 (4 x 4 MFMA tiles,
//     64 accumulator registers). 128 x 128 keeps the L2 re-reads of both operands near the bytes
//     stored (weights once per 128 pixels, pixels once per 128 rows) and still gives the s = 8
//     shapes (few pixels, thousands of rows) a grid of hundreds of workgroups.
//   * K is walked in chunks of 64 through LDS (2 x 16 KB, one buffer: K = cin is one to four
//     chunks, the launch is store-bound and several workgroups share a CU). Rows are 128 bytes, so
//     the 16-byte column of a row is XORed with row & 7: the ds_read_b128 fragment reads of 16
//     consecutive rows spread over all banks.
//   * weight rows are placed in LDS so that the MFMA tile pair (2p, 2p + 1) of a wave holds, in lane
//     group q = lane >> 4, rows 32p + 8q .. 32p + 8q + 7: a lane stores 8 consecutive output
//     channels of a pixel as one 16-byte vector straight from its registers.
//   * the K order is fixed (ascending chunks, the MFMA's own order inside), so results are
//     reproducible run to run; epilogue act(acc + bias), hardware round-to-nearest-even casts.
// f32 (parity mode): plain FMA, one thread per (pixel, 8 rows), ci ascending, one fmaf each.
#include "ycx_internal.h"

namespace {

constexpr int BR = 128;  // rows (tap, co) per workgroup
constexpr int BP = 128;  // low-resolution pixels per workgroup
constexpr int BK = 64;   // K elements per LDS chunk

struct DArgs {
  const void* x;
  const void* w;
  const float* bias;
  void* y;
  int M, H, W, Cin, in_coff, in_cs;
  int Cout, R, S, Ho, Wo, out_coff, out_cs;
  int act;
  float slope;
  int tiles_r;
};

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

// rows r .. r + 7 of one tap -> their 8 output channels of low-resolution pixel m
template <typename T>
__device__ __forceinline__ T* out_ptr(const DArgs& a, int m, int r) {
  const int tap = r / a.Cout, co = r - tap * a.Cout, dy = tap / a.S, dx = tap - dy * a.S;
  const int xw = m % a.W, t = m / a.W, yh = t % a.H, img = t / a.H;
  const size_t pix = ((size_t)img * a.Ho + (size_t)(yh * a.S + dy)) * a.Wo + (size_t)(xw * a.S + dx);
  return reinterpret_cast<T*>(a.y) + pix * a.out_cs + a.out_coff + co;
}

template <typename T>
__global__ __launch_bounds__(256) void deconv_mfma_kernel(DArgs a) {
  typedef __attribute__((ext_vector_type(8))) T tx8;
  __shared__ __attribute__((aligned(16))) T As[BR * BK];
  __shared__ __attribute__((aligned(16))) T Bs[BP * BK];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wp = wave & 1;  // the wave's 64 rows / 64 pixels of the tile
  const int rt = blockIdx.x % a.tiles_r, pt = blockIdx.x / a.tiles_r;
  const int r0 = rt * BR, m0 = pt * BP;
  const T* xg = reinterpret_cast<const T*>(a.x);
  const T* wg = reinterpret_cast<const T*>(a.w);

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  for (int k0 = 0; k0 < a.Cin; k0 += BK) {
    // 128 rows x 8 sixteen-byte columns per operand: four of each per thread (zero past R, M, cin)
    uint4 va[4], vb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = tid + 256 * u, row = i >> 3, k = k0 + (i & 7) * 8;
      va[u] = vb[u] = make_uint4(0u, 0u, 0u, 0u);
      if (k < a.Cin) {
        if (r0 + row < a.R) va[u] = *reinterpret_cast<const uint4*>(wg + (size_t)(r0 + row) * a.Cin + k);
        if (m0 + row < a.M)
          vb[u] = *reinterpret_cast<const uint4*>(xg + (size_t)(m0 + row) * a.in_cs + a.in_coff + k);
      }
    }
    if (k0) __syncthreads();  // the previous chunk's fragments have been read
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = tid + 256 * u, row = i >> 3, c = i & 7;
      // row 32p + 8q + 4t + j of the tile -> LDS row 32p + 16t + 4q + j (MFMA tile 2p + t, row 4q + j)
      const int ar = (row & ~31) | (((row >> 2) & 1) << 4) | (((row >> 3) & 3) << 2) | (row & 3);
      *reinterpret_cast<uint4*>(As + ar * BK + ((c ^ (ar & 7)) << 3)) = va[u];
      *reinterpret_cast<uint4*>(Bs + row * BK + ((c ^ (row & 7)) << 3)) = vb[u];
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < BK / 32; ++ks) {
      const int c = ks * 4 + (lane >> 4);  // lane l holds k = 8 (l >> 4) .. + 7 of the step
      tx8 af[4], bf[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = wr * 64 + i * 16 + (lane & 15);
        af[i] = *reinterpret_cast<const tx8*>(As + r * BK + ((c ^ (r & 7)) << 3));
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = wp * 64 + j * 16 + (lane & 15);
        bf[j] = *reinterpret_cast<const tx8*>(Bs + r * BK + ((c ^ (r & 7)) << 3));
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if constexpr (sizeof(T) == 2 && __is_same(T, _Float16))
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i], bf[j], acc[i][j], 0, 0, 0);
          else
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
    }
  }

  // ---- epilogue: C/D row = 4 (lane >> 4) + register, column = lane & 15 ----
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int r = r0 + wr * 64 + 32 * p + 8 * (lane >> 4);
    if (r >= a.R) continue;
    const float* bp = a.bias + r % a.Cout;
    const f32x4 b0 = *reinterpret_cast<const f32x4*>(bp), b1 = *reinterpret_cast<const f32x4*>(bp + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int m = m0 + wp * 64 + 16 * j + (lane & 15);
      if (m >= a.M) continue;
      float v[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = ycx_act<true>(acc[2 * p][j][e] + b0[e], a.act, a.slope);
        v[4 + e] = ycx_act<true>(acc[2 * p + 1][j][e] + b1[e], a.act, a.slope);
      }
      store8<T>(out_ptr<T>(a, m, r), v);
    }
  }
}

__global__ __launch_bounds__(256) void deconv_f32_kernel(DArgs a) {
  const int nv = a.R / 8;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)a.M * nv) return;
  const int m = (int)(idx / nv), r = (int)(idx - (long long)m * nv) * 8;
  const float* xp = reinterpret_cast<const float*>(a.x) + (size_t)m * a.in_cs + a.in_coff;
  const float* wp = reinterpret_cast<const float*>(a.w) + (size_t)r * a.Cin;
  float acc[8];
#pragma unroll
  for (int o = 0; o < 8; ++o) acc[o] = 0.0f;
  for (int k = 0; k < a.Cin; k += 4) {
    const f32x4 xv = *reinterpret_cast<const f32x4*>(xp + k);
#pragma unroll
    for (int o = 0; o < 8; ++o) {
      const f32x4 wv = *reinterpret_cast<const f32x4*>(wp + (size_t)o * a.Cin + k);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[o] = __builtin_fmaf(xv[e], wv[e], acc[o]);
    }
  }
  const float* bp = a.bias + r % a.Cout;
  float v[8];
#pragma unroll
  for (int o = 0; o < 8; ++o) v[o] = ycx_act<false>(acc[o] + bp[o], a.act, a.slope);
  store8<float>(out_ptr<float>(a, m, r), v);
}

}  // namespace

extern "C" ycx_status ycx_deconv2d(const ycx_conv_desc* d, const void* x, const void* w, const float* bias, void* y,
                                   void* stream) {
  YCX_CHECK_ARG(d);  // the descriptor is judged before the data pointers (checked below, before the launch)
  YCX_CHECK_ARG(d->n > 0 && d->h > 0 && d->w > 0 && d->cin > 0 && d->cout > 0 && d->ho > 0 && d->wo > 0);
  YCX_CHECK_ARG(d->kh > 0 && d->kw > 0 && d->stride > 0 && d->pad >= 0 && d->groups >= 0);
  YCX_CHECK_ARG((long long)d->ho == (long long)d->h * d->stride && (long long)d->wo == (long long)d->w * d->stride);
  YCX_CHECK_ARG(d->in_c_off >= 0 && d->in_c_off + d->cin <= d->in_c_stride);
  YCX_CHECK_ARG(d->out_c_off >= 0 && d->out_c_off + d->cout <= d->out_c_stride);
  const int s = d->stride;
  YCX_CHECK_SUPPORTED(d->kh == s && d->kw == s && (s == 2 || s == 4 || s == 8) && d->pad == 0);
  YCX_CHECK_DENSE(d);
  YCX_CHECK_SUPPORTED(d->dtype == YCX_DT_BF16 || d->dtype == YCX_DT_F16 || d->dtype == YCX_DT_F32);
  YCX_CHECK_SUPPORTED(d->act == YCX_ACT_NONE || d->act == YCX_ACT_SILU || d->act == YCX_ACT_LEAKY);
  YCX_CHECK_SUPPORTED(d->out_layout == YCX_OUT_NHWC && !d->in_pool && d->k_split <= 1);
  // 16-byte vectors of 16-bit channels on both sides (fp32: two per 8 channels)
  YCX_CHECK_SUPPORTED(d->cin % 8 == 0 && d->cout % 8 == 0 && d->in_c_off % 8 == 0 && d->in_c_stride % 8 == 0 &&
                      d->out_c_off % 8 == 0 && d->out_c_stride % 8 == 0);
  const long long M = (long long)d->n * d->h * d->w, R = (long long)s * s * d->cout;
  // M + BP and R + BR stay below 2^31: the tiles' row and pixel indices are ints
  YCX_CHECK_SUPPORTED(M < (1LL << 30) && (long long)d->n * d->ho * d->wo < (1LL << 31) && R < (1LL << 30));
  YCX_CHECK_ARG(x && w && bias && y);

  DArgs a;
  a.x = x; a.w = w; a.bias = bias; a.y = y;
  a.M = (int)M; a.H = d->h; a.W = d->w; a.Cin = d->cin; a.in_coff = d->in_c_off; a.in_cs = d->in_c_stride;
  a.Cout = d->cout; a.R = (int)R; a.S = s; a.Ho = d->ho; a.Wo = d->wo; a.out_coff = d->out_c_off;
  a.out_cs = d->out_c_stride;
  a.act = d->act; a.slope = d->leaky_slope;
  a.tiles_r = (int)((R + BR - 1) / BR);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (d->dtype == YCX_DT_F32) {
    const long long nwg = (M * (R / 8) + 255) / 256;
    YCX_CHECK_SUPPORTED(nwg < (1LL << 31));
    hipLaunchKernelGGL(deconv_f32_kernel, dim3((unsigned)nwg), dim3(256), 0, st, a);
    return ycx_launch_status();
  }
  const long long nwg = (long long)a.tiles_r * ((M + BP - 1) / BP);
  YCX_CHECK_SUPPORTED(nwg < (1LL << 31));
  if (d->dtype == YCX_DT_BF16)
    hipLaunchKernelGGL(deconv_mfma_kernel<__bf16>, dim3((unsigned)nwg), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(deconv_mfma_kernel<_Float16>, dim3((unsigned)nwg), dim3(256), 0, st, a);
  return ycx_launch_status();
}
