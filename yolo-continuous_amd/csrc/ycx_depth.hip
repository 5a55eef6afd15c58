// libycx_hip.so — space <-> depth moves on NHWC channel slices (ycx_space_depth): Contract, Expand and
// Focus's pixel-phase regrouping (nets/common.py:759-812) for an activation that is already in memory.
//
// A pure move: every element type is handled as bytes (16-byte vectors; 8-byte ones for e4m3 slices on
// 8-channel bounds), so NaN payloads, -0.0 and every e4m3 code pass through unchanged. The flat index
// runs over the OUTPUT vectors, channel fastest: consecutive lanes store consecutive vectors of a pixel's
// slice and the store side is fully coalesced whatever the mode; the load side then reads whole channel
// runs (C for Contract / Focus, C / s^2 for Expand), each run contiguous in the input. No LDS, no scratch.
#include "ycx_internal.h"

namespace {

struct SDArgs {
  const void* x;
  void* y;
  int h, w;          // input map
  int ho, wo;        // output map
  int s;             // gain
  int rv;            // vectors per contiguous channel run
  int ocv;           // vectors per output pixel slice (Contract / Focus: s*s*rv, Expand: rv)
  long long in_off, in_stride, out_off, out_stride;  // channel offset / pixel stride, in vectors
  long long total;   // n * ho * wo * ocv
};

// I: the type the flat index is decomposed in -- uint32_t when the vector count fits (one 32-bit
// division per coordinate), long long otherwise. Addresses are 64-bit either way.
template <typename V, int MODE, typename I>
__global__ void __launch_bounds__(256) space_depth_kernel(SDArgs a) {
  const V* __restrict__ x = reinterpret_cast<const V*>(a.x);
  V* __restrict__ y = reinterpret_cast<V*>(a.y);
  const int s = a.s, rv = a.rv;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < a.total;
       i += (long long)gridDim.x * blockDim.x) {
    const I fi = (I)i;
    const int cv = (int)(fi % (I)a.ocv);
    const I p = fi / (I)a.ocv;
    const int ox = (int)(p % (I)a.wo);
    const I t = p / (I)a.wo;
    const int oy = (int)(t % (I)a.ho);
    const long long n = (long long)(t / (I)a.ho);
    int iy, ix, icv;
    if (MODE == YCX_SD_EXPAND) {  // y[n, h*s+a, w*s+b, c'] = x[n, h, w, (a*s+b)*C' + c']
      iy = oy / s;
      ix = ox / s;
      icv = ((oy - iy * s) * s + (ox - ix * s)) * rv + cv;
    } else {
      const int q = cv / rv;  // the pixel phase this run comes from
      icv = cv - q * rv;
      int pa, pb;
      if (MODE == YCX_SD_FOCUS) {  // y[.., (2*b+a)*C + c] = x[n, 2*ho+a, 2*wo+b, c]: the row phase varies fastest
        pa = q & 1;
        pb = q >> 1;
      } else {                     // y[.., (a*s+b)*C + c] = x[n, ho*s+a, wo*s+b, c]
        pa = q / s;
        pb = q - pa * s;
      }
      iy = oy * s + pa;
      ix = ox * s + pb;
    }
    const V v = x[((n * a.h + iy) * a.w + ix) * a.in_stride + a.in_off + icv];
    y[((n * a.ho + oy) * a.wo + ox) * a.out_stride + a.out_off + cv] = v;
  }
}

unsigned sd_grid(long long total) {
  long long b = (total + 255) / 256;
  if (b > 256LL * 8) b = 256LL * 8;  // 8 blocks per CU, grid-stride beyond
  return (unsigned)(b < 1 ? 1 : b);
}

template <typename V, int MODE>
void sd_launch(const SDArgs& a, hipStream_t st) {
  if (a.total <= 0xffffffffLL)
    hipLaunchKernelGGL((space_depth_kernel<V, MODE, uint32_t>), dim3(sd_grid(a.total)), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((space_depth_kernel<V, MODE, long long>), dim3(sd_grid(a.total)), dim3(256), 0, st, a);
}

template <typename V>
void sd_launch_mode(int mode, const SDArgs& a, hipStream_t st) {
  if (mode == YCX_SD_CONTRACT) sd_launch<V, YCX_SD_CONTRACT>(a, st);
  else if (mode == YCX_SD_EXPAND) sd_launch<V, YCX_SD_EXPAND>(a, st);
  else sd_launch<V, YCX_SD_FOCUS>(a, st);
}

}  // namespace

extern "C" ycx_status ycx_space_depth(const ycx_depth_desc* d, const void* x, void* y, void* stream) {
  YCX_CHECK_ARG(d);  // the descriptor is judged before the data pointers (checked below, before the launch)
  YCX_CHECK_ARG(d->n > 0 && d->h > 0 && d->w > 0 && d->c > 0 && d->ho > 0 && d->wo > 0);
  YCX_CHECK_ARG(d->in_c_off >= 0 && d->out_c_off >= 0 && d->in_c_stride > 0 && d->out_c_stride > 0);
  YCX_CHECK_SUPPORTED(d->mode == YCX_SD_CONTRACT || d->mode == YCX_SD_EXPAND || d->mode == YCX_SD_FOCUS);
  YCX_CHECK_SUPPORTED(d->gain >= 2 && d->gain <= 4 && (d->mode != YCX_SD_FOCUS || d->gain == 2));
  YCX_CHECK_SUPPORTED(d->dtype == YCX_DT_BF16 || d->dtype == YCX_DT_F16 || d->dtype == YCX_DT_F32 ||
                      d->dtype == YCX_DT_FP8);
  const int s = d->gain, ss = s * s;
  long long run, out_c;  // the contiguous channel run, and the output slice's width
  if (d->mode == YCX_SD_EXPAND) {
    YCX_CHECK_ARG(d->c % ss == 0);
    YCX_CHECK_ARG(d->ho == (long long)d->h * s && d->wo == (long long)d->w * s);
    run = out_c = d->c / ss;
  } else {
    YCX_CHECK_ARG(d->h % s == 0 && d->w % s == 0);
    YCX_CHECK_ARG(d->ho == d->h / s && d->wo == d->w / s);
    run = d->c;
    out_c = (long long)d->c * ss;
  }
  YCX_CHECK_ARG((long long)d->in_c_off + d->c <= d->in_c_stride);
  YCX_CHECK_ARG(d->out_c_off + out_c <= d->out_c_stride);
  // runs, offsets and strides in multiples of 8 elements, the granularity of every slice the plan makes
  YCX_CHECK_SUPPORTED(run % 8 == 0 && d->in_c_off % 8 == 0 && d->in_c_stride % 8 == 0 && d->out_c_off % 8 == 0 &&
                      d->out_c_stride % 8 == 0);
  YCX_CHECK_ARG(x && y);
  if (x == y) {  // two slices of one buffer: the same pixel stride and disjoint channel ranges only
    YCX_CHECK_ARG(d->in_c_stride == d->out_c_stride);
    YCX_CHECK_ARG(d->in_c_off + d->c <= d->out_c_off || d->out_c_off + out_c <= d->in_c_off);
  }

  const int esz = d->dtype == YCX_DT_F32 ? 4 : d->dtype == YCX_DT_FP8 ? 1 : 2;
  // bytes per vector: 16, or 8 for an e4m3 slice that sits on 8- but not 16-channel bounds
  const bool v16 = esz > 1 || (run % 16 == 0 && d->in_c_off % 16 == 0 && d->in_c_stride % 16 == 0 &&
                               d->out_c_off % 16 == 0 && d->out_c_stride % 16 == 0);
  const int ve = (v16 ? 16 : 8) / esz;  // elements per vector
  SDArgs a;
  a.x = x; a.y = y;
  a.h = d->h; a.w = d->w; a.ho = d->ho; a.wo = d->wo; a.s = s;
  a.rv = (int)(run / ve);
  a.ocv = (int)(out_c / ve);
  a.in_off = d->in_c_off / ve; a.in_stride = d->in_c_stride / ve;
  a.out_off = d->out_c_off / ve; a.out_stride = d->out_c_stride / ve;
  a.total = (long long)d->n * d->ho * d->wo * a.ocv;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (v16) sd_launch_mode<uint4>(d->mode, a, st);
  else sd_launch_mode<uint2>(d->mode, a, st);
  return ycx_launch_status();
}
