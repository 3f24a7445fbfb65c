// The LDS-resident Stockham autosort FFT shared by metrics.hip (forward STFT and its reductions) and splice.hip (forward
// and inverse transforms): radix 4 with a closing radix-2 pass when log2 N is odd, between two LDS buffers of G frames of
// N float2 each.  Every pass reads float2 at unit stride over the lanes (no bank conflict) and writes at j0 + r Ns: unit
// stride from Ns = 16 on.  The first pass has no twiddles: the caller forms its four inputs (from memory or from LDS) and
// hands them to fft_first_pass; fft_later_passes runs the rest with the per-pass twiddle tables staged in LDS, indexed
// [r - 1][k] so that lanes read consecutive entries.  The transform is the forward one, X[k] = sum_i x[i] e^{-2 pi i k i / N};
// the inverse goes through the same passes and tables as ifft(Z) = conj(fft(conj Z)) / N.
#pragma once
#include "jat_metrics_kernels.h"

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }

// forward 4-point DFT: o[r] = sum_q v[q] (-i)^(r q)
__device__ __forceinline__ void dft4(float2 v0, float2 v1, float2 v2, float2 v3, float2* o) {
  const float2 a0 = cadd(v0, v2), a1 = csub(v0, v2), a2 = cadd(v1, v3), d = csub(v1, v3);
  const float2 a3 = make_float2(d.y, -d.x);   // -i (v1 - v3)
  o[0] = cadd(a0, a2);
  o[1] = cadd(a1, a3);
  o[2] = csub(a0, a2);
  o[3] = csub(a1, a3);
}

// pass 0 (Ns = 1, no twiddles) of one frame: v[r] is the input at j + r N / 4, j < N / 4; the four outputs go to
// frame[4 j .. 4 j + 3] as 32 contiguous bytes
__device__ __forceinline__ void fft_first_pass(const float2* v, float2* frame, int j) {
  float2 o[4];
  dft4(v[0], v[1], v[2], v[3], o);
  float4* dst = (float4*)(frame + 4 * j);
  dst[0] = make_float4(o[0].x, o[0].y, o[1].x, o[1].y);
  dst[1] = make_float4(o[2].x, o[2].y, o[3].x, o[3].y);
}

// passes 1 .. n_pass - 1 over the G frames that pass 0 left in buf0 (a barrier must lie between); tw is the LDS copy of the
// twiddle table.  Every thread of the block calls it.  Returns the buffer that holds the spectra; *other is the free one.
// Ends on a barrier.
__device__ __forceinline__ float2* fft_later_passes(const MetricsPlan& p, const float2* tw, float2* buf0, float2* buf1, int G,
                                                    int tid, float2** other) {
  const int N = p.n_fft, q = N >> 2, lq = 31 - __clz(q);
  float2* src = buf0;
  float2* dst = buf1;
  for (int ps = 1; ps < p.n_pass; ++ps) {
    const int ns = p.ns[ps], sh = 31 - __clz(ns);
    const float2* tp = tw + p.off[ps];
    if (p.radix[ps] == 4) {
      for (int jj = tid; jj < G * q; jj += MT_THREADS) {
        const int g = jj >> lq, j = jj & (q - 1), k = j & (ns - 1);
        const float2* sp = src + g * N + j;
        const float2 v0 = sp[0], v1 = cmul(sp[q], tp[k]), v2 = cmul(sp[2 * q], tp[ns + k]), v3 = cmul(sp[3 * q], tp[2 * ns + k]);
        float2 o[4];
        dft4(v0, v1, v2, v3, o);
        float2* dp = dst + g * N + (((j >> sh) << (sh + 2)) | k);
        dp[0] = o[0];
        dp[ns] = o[1];
        dp[2 * ns] = o[2];
        dp[3 * ns] = o[3];
      }
    } else {
      const int h = N >> 1, lh = lq + 1;
      for (int jj = tid; jj < G * h; jj += MT_THREADS) {
        const int g = jj >> lh, j = jj & (h - 1), k = j & (ns - 1);
        const float2* sp = src + g * N + j;
        const float2 v0 = sp[0], v1 = cmul(sp[h], tp[k]);
        float2* dp = dst + g * N + (((j >> sh) << (sh + 1)) | k);
        dp[0] = cadd(v0, v1);
        dp[ns] = csub(v0, v1);
      }
    }
    __syncthreads();
    float2* x = src;
    src = dst;
    dst = x;
  }
  *other = dst;
  return src;
}
