// Voicing-aware index rates for gfx950: the stability classes of a pitch track, the per-frame rate track they
// select, and the blend's last line with that track in the place of the scalar rate.  fp32 and integers throughout, every
// operation rounded once (nothing fused but the mix's one fma, below), no atomics: tests/retrieval_rate_ref.py restates the
// three kernels bit for bit, and the bits do not depend on B, on the grid or on the run.  The search and the blends that
// produce the retrieved track are the kernels of retrieval.hip, retrieval_ms.hip and retrieval_ivf.hip, unchanged.
//
// Classes.  Frame j is LIVE when voiced[j] != 0 and f0[j] is positive and finite.  For a live frame t,
//   count[t] = #{ j in [max(0, t - W), min(F - 1, t + W)] : j live, f0[j] <= f0[t] * ratio, f0[t] <= f0[j] * ratio },
// t included, each product one fp32 multiply (it may round to +inf, which every finite f0 is below).  count = 0 on a frame that is
// not live.  cls = 0 (not live), 1 (count < min_count), 2 (count >= min_count).
//
// Rate track.  c[t] = table[min(cls[t], 2)] for t < F and table[0] behind the pitch track.  With a = max(0, t - S),
// b = min(T - 1, t + S), n = b - a + 1:
//   r[t] = clamp(c[t] + (((c[a] - c[t]) + (c[a+1] - c[t])) + ... + (c[b] - c[t])) / float(n), 0, 1).
// The mean is taken of DIFFERENCES: where the window holds one class every difference is +0 and r[t] = c[t] exactly, which a
// mean of the values themselves (n c / n) does not promise.
//
// Mix.  y = fma(1 - r, x, r v) with r = rates[b, t]: 1 - r and r v rounded once each, then one fma.  This is what
// bank_blend_kernel's last line compiles to and what bank_mix_scales_kernel writes out (see the top of retrieval_ms.hip), so a
// constant track gives the bits of the scalar blend.
//
// All three kernels stream with lanes along t: every input byte comes from HBM once (the halo of a class tile and the 2 S + 1
// taps of the smoothing are shared between neighbouring lanes through LDS and the cache) and every output byte is written once.
#include "jat_retrieval_rate_kernels.h"

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ float add1(float a, float b) { return a + b; }
__device__ __forceinline__ float sub1(float a, float b) { return a - b; }
__device__ __forceinline__ float mul1(float a, float b) { return a * b; }
__device__ __forceinline__ float div1(float a, float b) { return a / b; }   // correctly rounded (hipcc's default for fp32 /)

// ---- stability classes --------------------------------------------------------------------------------------------------------
// One workgroup per row.  A tile is RT_THREADS frames plus W frames of halo on either side; LDS holds g[j] = f0[j] where j is
// live and 0 elsewhere (outside the row too), so "j is live" is g[j] > 0 and the window needs no clipping of its own.
__global__ __launch_bounds__(RT_THREADS) void f0_classes_kernel(const float* __restrict__ f0, const uint8_t* __restrict__ voiced,
                                                                int F, int W, float ratio, int min_count,
                                                                uint8_t* __restrict__ cls, int32_t* __restrict__ count,
                                                                int32_t* __restrict__ summary) {
  __shared__ float g[RT_THREADS + 2 * RR_MAX_HALF_WINDOW];
  __shared__ int red[2][RT_THREADS];
  const int tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * (size_t)F;
  int n_live = 0, n_stable = 0;
  for (int t0 = 0; t0 < F; t0 += RT_THREADS) {
    for (int e = tid; e < RT_THREADS + 2 * W; e += RT_THREADS) {
      const int j = t0 - W + e;
      float v = 0.f;
      if (j >= 0 && j < F && voiced[base + j] != 0) {
        const float f = f0[base + j];
        if (f > 0.f && f < __builtin_inff()) v = f;                    // a NaN fails the first test
      }
      g[e] = v;
    }
    __syncthreads();
    const int t = t0 + tid;
    if (t < F) {
      const float ft = g[tid + W];
      int n = 0;
      if (ft > 0.f) {
        const float hi = mul1(ft, ratio);
        for (int e = 0; e <= 2 * W; ++e) {
          const float fj = g[tid + e];
          n += (fj > 0.f && fj <= hi && ft <= mul1(fj, ratio)) ? 1 : 0;
        }
      }
      const int c = ft > 0.f ? (n >= min_count ? 2 : 1) : 0;
      cls[base + t] = (uint8_t)c;
      if (count) count[base + t] = n;
      n_live += c > 0, n_stable += c == 2;
    }
    __syncthreads();
  }
  if (!summary) return;
  red[0][tid] = n_live, red[1][tid] = n_stable;
  __syncthreads();
  for (int off = RT_THREADS / 2; off > 0; off >>= 1) {
    if (tid < off) red[0][tid] += red[0][tid + off], red[1][tid] += red[1][tid + off];
    __syncthreads();
  }
  if (tid < 2) summary[(size_t)blockIdx.x * 2 + tid] = red[tid][0];
}

// ---- rate track ---------------------------------------------------------------------------------------------------------------
struct RateTable { float r[3]; };

__device__ __forceinline__ float table_at(const uint8_t* __restrict__ cls, int F, int j, const RateTable& tb) {
  if (j >= F) return tb.r[0];                                          // behind the pitch track: unvoiced
  const int c = cls[j];
  return c >= 2 ? tb.r[2] : (c == 1 ? tb.r[1] : tb.r[0]);
}

__global__ __launch_bounds__(RT_THREADS) void rate_track_kernel(const uint8_t* __restrict__ cls, int F, int T, RateTable tb, int S,
                                                                float* __restrict__ r) {
  const int t = blockIdx.x * RT_THREADS + threadIdx.x;
  if (t >= T) return;
  const uint8_t* row = cls + (size_t)blockIdx.y * (size_t)F;
  const float ct = table_at(row, F, t, tb);
  const int a = max(0, t - S), b = min(T - 1, t + S);
  float acc = sub1(table_at(row, F, a, tb), ct);
  for (int j = a + 1; j <= b; ++j) acc = add1(acc, sub1(table_at(row, F, j, tb), ct));
  const float v = add1(ct, div1(acc, (float)(b - a + 1)));
  r[(size_t)blockIdx.y * (size_t)T + t] = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
}

// ---- mix ------------------------------------------------------------------------------------------------------------------------
// Lanes along t, the rate of a frame read once per thread; RR_MIX_ROWS channel rows are loaded before the first is written.
// x, v and y are not restrict: y may be x or v (a thread reads exactly the elements it writes, before it writes them).
__global__ __launch_bounds__(RT_THREADS) void rate_mix_kernel(const float* x, const float* v, const float* __restrict__ rates,
                                                              float* y, int C, int T) {
  const int t = blockIdx.x * RT_THREADS + threadIdx.x;
  if (t >= T) return;
  const int b = blockIdx.z;
  const float rate = rates[(int64_t)b * T + t];
  const float keep = sub1(1.f, rate);
  for (int64_t c0 = (int64_t)blockIdx.y * RR_MIX_ROWS; c0 < C; c0 += (int64_t)gridDim.y * RR_MIX_ROWS) {
    float xs[RR_MIX_ROWS], vs[RR_MIX_ROWS];
#pragma unroll
    for (int k = 0; k < RR_MIX_ROWS; ++k) {
      const int64_t off = ((int64_t)b * C + c0 + k) * T + t;
      xs[k] = c0 + k < C ? x[off] : 0.f;
      vs[k] = c0 + k < C ? v[off] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < RR_MIX_ROWS; ++k) {
      const int64_t off = ((int64_t)b * C + c0 + k) * T + t;
      if (c0 + k < C) y[off] = fmaf(keep, xs[k], mul1(rate, vs[k]));   // r v rounded, then the one fma
    }
  }
}

}  // namespace

hipError_t f0_classes_launch(const float* f0, const uint8_t* voiced, int B, int F, int W, float ratio, int min_count,
                             uint8_t* cls, int32_t* count, int32_t* summary, hipStream_t s) {
  hipLaunchKernelGGL(f0_classes_kernel, dim3((unsigned)B), dim3(RT_THREADS), 0, s, f0, voiced, F, W, ratio, min_count, cls, count,
                     summary);
  return hipGetLastError();
}

hipError_t rate_track_launch(const uint8_t* cls, int B, int F, int T, float r0, float r1, float r2, int S, float* r,
                             hipStream_t s) {
  const RateTable tb = {{r0, r1, r2}};
  const dim3 grid((unsigned)((T + RT_THREADS - 1) / RT_THREADS), (unsigned)B);
  hipLaunchKernelGGL(rate_track_kernel, grid, dim3(RT_THREADS), 0, s, cls, F, T, tb, S, r);
  return hipGetLastError();
}

hipError_t rate_mix_launch(const float* x, const float* v, const float* rates, float* y, int B, int C, int T, hipStream_t s) {
  const int groups = (C + RR_MIX_ROWS - 1) / RR_MIX_ROWS;
  const dim3 grid((unsigned)((T + RT_THREADS - 1) / RT_THREADS), (unsigned)(groups < 65535 ? groups : 65535), (unsigned)B);
  hipLaunchKernelGGL(rate_mix_kernel, grid, dim3(RT_THREADS), 0, s, x, v, rates, y, C, T);
  return hipGetLastError();
}
