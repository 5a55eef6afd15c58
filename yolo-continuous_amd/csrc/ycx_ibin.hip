// IBin eval branch for one level on gfx950 (nets/ibin.py:48-72, with the strides the reference
// leaves unset supplied by the caller): the raw map re-laid as (bs, na, ny, nx, no) and the decoded
// rows z (pixel units, nc + 5 wide). Width and height are not regressed directly: each has one
// regression logit and bin_count bin logits, and SigmoidBin.forward (losses/sigmoid_bin.py:49-63)
// picks the bin centre of the largest sigmoid'd bin score and adds the regression term:
//
//   p      = sigmoid(raw)                                  all no columns
//   xy     = (p[0:2] * 2 - 0.5 + grid) * stride
//   w      = clamp((p[2] * 2 - 1) * step + w_bins[argmax p[3:3+B]], 0, 4) * anchor_w
//   h      = clamp((p[3+B] * 2 - 1) * step + h_bins[argmax p[4+B:4+2B]], 0, 4) * anchor_h
//   z      = xy, w, h, p[2 * (B + 1) + 2:]                 B = bin_count = 21
//
// Bit-exactness: the fp32 expressions and their order restate the reference operation by
// operation; FMA contraction is off so every product and sum rounds as the CPU code does. The
// arg-max is taken over the sigmoid'd scores, as the reference does (two distinct logits can round
// to one score), with torch.max's rule: the first index of the maximum, a NaN beating everything.
#pragma clang fp contract(off)
#include <stdint.h>
#include "ycx_internal.h"

namespace {

constexpr int kBins = 21;            // the reference's eval slices are written out for 21 bins
constexpr int kGroup = kBins + 1;    // SigmoidBin.get_length(): one regression logit + the bins
constexpr float kBinMin = 0.0f, kBinMax = 4.0f;
constexpr size_t kLdsBudget = 64 * 1024;

// Both bin tables travel in the kernel's arguments (2 x 21 floats): no device allocation, no copy.
struct ibin_tables {
  float w[kBins];
  float h[kBins];
};

// q = i / n, r = i % n for 0 <= i < 2^14 and 0 < n <= 256, through one fp32 multiply: (i + 0.5) / n
// is at least 0.5 / 256 away from every integer, far more than the 2^-22 relative error of the
// product, so the truncation is exact (a runtime integer division would cost ~25 VALU ops per
// stored element in a kernel that has nothing else to hide behind).
__device__ __forceinline__ void split(int i, int n, float inv_n, int& q, int& r) {
  q = (int)(((float)i + 0.5f) * inv_n);
  r = i - q * n;
}

// Block = CELLS consecutive grid cells of one (n, a). Phase 1 reads the NCHW head channel by
// channel (coalesced over cells) into two LDS tiles, raw and sigmoid'd, row stride ld = no | 1
// floats (odd: a column write by 32 consecutive cells touches 32 different banks). Phase 2: one lane
// per (cell, w | h) scans its 21 bin scores in the LDS row and overwrites its own regression slot
// with the decoded size (no other lane reads that slot). Phase 3 stores the z and xview rows of the
// block as contiguous runs.
template <int CELLS>
__global__ void __launch_bounds__(256) ibin_kernel(ycx_decode_desc d, float stride, ibin_tables bins,
                                                   const float* __restrict__ head, float* __restrict__ z,
                                                   float* __restrict__ xview) {
  extern __shared__ __attribute__((aligned(16))) float tile[];  // [2][CELLS][ld]
  const int n = blockIdx.z, a = blockIdx.y;
  const int hw = d.h * d.w, no = d.no, ld = no | 1;
  const int cell0 = blockIdx.x * CELLS;
  const int ncell = min(CELLS, hw - cell0);
  float* sig = tile;
  float* raw = tile + CELLS * ld;
  const float* hb = head + ((size_t)n * d.na * no + (size_t)a * no) * hw;
  {
    // a thread keeps one cell and walks the channels o0, o0 + kStep, ...: no index division, and the
    // unrolled loop has eight independent loads in flight per lane
    constexpr int kStep = 256 / CELLS;
    const int c = threadIdx.x % CELLS, o0 = threadIdx.x / CELLS;
    if (c < ncell) {
      const int cell = cell0 + c;
      const float* src = hb + cell;
      float* ps = sig + c * ld;
      float* pr = raw + c * ld;
#pragma unroll 8
      for (int o = o0; o < no; o += kStep) {
        const float r = src[(size_t)o * hw];
        pr[o] = r;
        ps[o] = ycx_sigmoid(r);
      }
      if (o0 < 2) {  // kStep >= 4: the thread that wrote column 0 (x) or 1 (y) of this cell decodes it
        const float g = o0 == 0 ? (float)(cell % d.w) : (float)(cell / d.w);
        ps[o0] = ((ps[o0] * 2.0f) - 0.5f + g) * stride;
      }
    }
  }
  __syncthreads();
  // lanes [0, CELLS): widths, lanes [CELLS, 2 CELLS): heights, so the 32 lanes of a half wave read
  // one column of 32 different rows (conflict-free at an odd row stride)
  if (threadIdx.x < 2 * CELLS) {
    const int which = threadIdx.x / CELLS, c = threadIdx.x - which * CELLS;
    if (c < ncell) {
      float* g = sig + c * ld + 2 + which * kGroup;  // [0] regression, [1 .. kBins] bin scores
      float best = g[1];
      int bi = 0;
#pragma unroll
      for (int k = 1; k < kBins; ++k) {
        const float v = g[1 + k];
        const bool up = v > best || (v != v && best == best);  // strictly larger, or the first NaN
        best = up ? v : best;
        bi = up ? k : bi;
      }
      float centre = 0.0f;  // a select chain over the argument table: no indexed copy, no scratch
#pragma unroll
      for (int k = 0; k < kBins; ++k) centre = bi == k ? (which ? bins.h[k] : bins.w[k]) : centre;
      const float step = (float)((double)(kBinMax - kBinMin) / kBins);  // SigmoidBin.step, cast by the fp32 multiply
      float v = ((g[0] * 2.0f) - 1.0f) * step + centre;
      v = v < kBinMin ? kBinMin : v;  // torch.clamp: a NaN stays a NaN
      v = v > kBinMax ? kBinMax : v;
      g[0] = v * d.anchors_scaled[2 * a + which];
    }
  }
  __syncthreads();
  const int nz = no - 2 * kGroup + 2;  // nc + 5
  const size_t row0 = (size_t)a * hw + cell0;  // (a, y, x) order = view(bs, -1, nz) of (bs, na, ny, nx, nz)
  float* zb = z + ((size_t)n * d.rows_total + d.row_off + row0) * nz;
  float* xb = xview + ((size_t)n * d.na * hw + row0) * no;
  const float inv_nz = 1.0f / (float)nz, inv_no = 1.0f / (float)no;
  for (int idx = threadIdx.x; idx < ncell * nz; idx += blockDim.x) {
    int c, j;
    split(idx, nz, inv_nz, c, j);
    // z columns: x, y, w (the width group's slot 0), h (the height group's), then objectness and classes
    const int col = j < 3 ? j : (j == 3 ? 2 + kGroup : j + 2 * kGroup - 2);
    zb[idx] = sig[c * ld + col];
  }
  if (ld == no) {
    for (int idx = threadIdx.x; idx < ncell * no; idx += blockDim.x) xb[idx] = raw[idx];
  } else {
    for (int idx = threadIdx.x; idx < ncell * no; idx += blockDim.x) {
      int c, j;
      split(idx, no, inv_no, c, j);
      xb[idx] = raw[c * ld + j];
    }
  }
}

template <int CELLS>
void launch(const ycx_decode_desc* d, float stride, const ibin_tables& bins, const float* head, float* z,
            float* xview, void* stream) {
  const size_t lds = (size_t)2 * CELLS * (d->no | 1) * sizeof(float);
  dim3 grid(ycx_cdiv((long long)d->h * d->w, CELLS), d->na, d->n);
  hipLaunchKernelGGL(ibin_kernel<CELLS>, grid, dim3(256), lds, reinterpret_cast<hipStream_t>(stream), *d, stride,
                     bins, head, z, xview);
}

}  // namespace

extern "C" ycx_status ycx_ibin_decode(const ycx_decode_desc* d, float stride, int32_t bin_count, const float* w_bins,
                                      const float* h_bins, const float* head, float* z, float* xview, void* stream) {
  YCX_CHECK_ARG(d != nullptr);
  YCX_CHECK_ARG(d->n > 0 && d->h > 0 && d->w > 0 && d->na > 0 && d->no > 0 && bin_count > 0);
  YCX_CHECK_SUPPORTED(d->na <= 8 && d->n <= 65535);
  YCX_CHECK_SUPPORTED(bin_count == kBins);  // nets/ibin.py:62-70 slices 2:24, 24:46, 46: by hand
  YCX_CHECK_ARG(d->no > 2 * (bin_count + 1) + 3);  // at least one class
  YCX_CHECK_ARG(d->row_off >= 0 && (long long)d->row_off + (long long)d->na * d->h * d->w <= d->rows_total);
  YCX_CHECK_SUPPORTED(d->no <= 256);
  YCX_CHECK_ARG(w_bins && h_bins && head && z && xview);
  ibin_tables bins;
  for (int k = 0; k < kBins; ++k) {
    bins.w[k] = w_bins[k];
    bins.h[k] = h_bins[k];
  }
  // cells per block: the largest of 64, 32, 16 whose two tiles stay inside 64 KB of dynamic LDS
  // (no = 127: 64 cells = 65024 B; no = 256: 16 cells = 32896 B)
  const size_t row_bytes = (size_t)2 * (d->no | 1) * sizeof(float);
  if (64 * row_bytes <= kLdsBudget) launch<64>(d, stride, bins, head, z, xview, stream);
  else if (32 * row_bytes <= kLdsBudget) launch<32>(d, stride, bins, head, z, xview, stream);
  else launch<16>(d, stride, bins, head, z, xview, stream);
  return ycx_launch_status();
}
