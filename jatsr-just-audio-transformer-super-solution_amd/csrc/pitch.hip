// Pitch tracking (YIN, de Cheveigne & Kawahara 2002, steps 1-5) and the comparison of two F0 tracks; the definitions are in
// include/jat_hip.h and, in fp64, in tests/pitch_ref.py.  fp32 in both operand-dtype builds, no atomics.
//
// yin_kernel.  One block takes one frame at a time: the zero-padded frame goes to LDS, the difference function
//   d(tau) = sum_{j < W} (x[j] - x[j + tau])^2
// is summed in its direct form (non-negative terms: nothing cancels at a periodic signal's dip, which is the value the
// threshold and the interpolation read).  A thread owns PT_LAGS = 4 consecutive lags tau0 .. tau0 + 3 with tau0 a multiple
// of 4, so the samples x[j + tau0 ..] it needs for four j are two aligned 16-byte LDS slots of which one is carried over
// from the step before: per 16 terms a thread issues one 16-byte read of its own (consecutive lanes read consecutive slots)
// and one 16-byte broadcast read of x[j .. j + 3].  The compiler pairs the 16 subtracts and 16 fmas into packed fp32
// instructions; left alone it also re-reads the window as shifted 8-byte pairs, which made the loop LDS-bound (measured:
// 306 us against 243 us for 47.6 s of audio), so the window read is made opaque to it.  Each lag has one accumulator and
// adds its terms in ascending j.  d stays in LDS; the running sum of the cumulative mean is a block scan in
// a fixed shape (PT_THREADS contiguous chunks, each summed in order, a Hillis-Steele scan of the chunk totals); one pass
// finds the first trough under the threshold and the lowest-index minimum; thread 0 interpolates and writes the outputs.
#include <float.h>
#include <limits.h>
#include <math.h>

#include "jat_pitch_kernels.h"

extern __shared__ __align__(16) float pt_lds[];

__global__ void __launch_bounds__(PT_THREADS)
yin_kernel(YinPlan p, const float* __restrict__ x, int64_t L, int frames, int64_t work, float* __restrict__ f0,
           float* __restrict__ aperiodicity, uint8_t* __restrict__ voiced, int32_t* __restrict__ index,
           float* __restrict__ d_out, float* __restrict__ c_out) {
  constexpr int T = PT_THREADS;
  const int tid = threadIdx.x;
  const int FL = p.frame_length, W = p.W, MP = p.max_period;
  const int NX = (FL + 3) / 4 * 4 + PT_PAD;
  float* xs = pt_lds;          // [NX] the frame, zeros behind it
  float* dl = pt_lds + NX;     // [MP + 1] d, then the cumulative-mean-normalised difference in place
  __shared__ float s_val[T];
  __shared__ int s_idx[T], s_first[T];

  for (int64_t w = blockIdx.x; w < work; w += gridDim.x) {
    const int64_t b = w / frames;
    const int f = (int)(w - b * frames);
    const float* row = x + (size_t)b * (size_t)L;
    const int64_t first_sample = (int64_t)f * p.hop - FL / 2;
    __syncthreads();                                          // the frame before is no longer read
    for (int i = tid; i < NX; i += T) {
      const int64_t q = first_sample + i;
      xs[i] = (i < FL && q >= 0 && q < L) ? row[q] : 0.f;
    }
    __syncthreads();

    // d(tau), tau = 0 .. MP.  Highest index read: (W & ~3) - 4 + (MP & ~3) + 7 <= W + MP + 3 <= FL + 2 < NX.
    const int Wq = W & ~3;
    for (int t0 = tid * PT_LAGS; t0 <= MP; t0 += T * PT_LAGS) {
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
      float4 lo = *(const float4*)&xs[t0];
      for (int j = 0; j < Wq; j += 4) {
        const float4 xj = *(const float4*)&xs[j];
        float4 hi = *(const float4*)&xs[j + t0 + 4];
        asm volatile("" : "+v"(hi.x), "+v"(hi.y), "+v"(hi.z), "+v"(hi.w));   // one 16-byte read, no shifted re-reads
        const float win[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        const float xv[4] = {xj.x, xj.y, xj.z, xj.w};
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          float e;
          e = xv[jj] - win[jj + 0], a0 = fmaf(e, e, a0);
          e = xv[jj] - win[jj + 1], a1 = fmaf(e, e, a1);
          e = xv[jj] - win[jj + 2], a2 = fmaf(e, e, a2);
          e = xv[jj] - win[jj + 3], a3 = fmaf(e, e, a3);
        }
        lo = hi;
      }
      for (int j = Wq; j < W; ++j) {                          // W is no multiple of 4: at most three more terms per lag
        const float v = xs[j];
        float e;
        e = v - xs[j + t0 + 0], a0 = fmaf(e, e, a0);
        e = v - xs[j + t0 + 1], a1 = fmaf(e, e, a1);
        e = v - xs[j + t0 + 2], a2 = fmaf(e, e, a2);
        e = v - xs[j + t0 + 3], a3 = fmaf(e, e, a3);
      }
      dl[t0] = a0;
      if (t0 + 1 <= MP) dl[t0 + 1] = a1;
      if (t0 + 2 <= MP) dl[t0 + 2] = a2;
      if (t0 + 3 <= MP) dl[t0 + 3] = a3;
    }
    __syncthreads();

    // running sum of d(1 .. MP): thread t owns lags 1 + t C .. 1 + t C + C - 1
    const int C = (MP + T - 1) / T;
    const int lag_lo = 1 + tid * C, lag_hi = min(MP, lag_lo + C - 1);
    float part = 0.f;
    for (int t = lag_lo; t <= lag_hi; ++t) part += dl[t];
    s_val[tid] = part;
    __syncthreads();
    for (int off = 1; off < T; off <<= 1) {
      const float v = tid >= off ? s_val[tid - off] : 0.f;
      __syncthreads();
      if (tid >= off) s_val[tid] += v;
      __syncthreads();
    }
    float run = tid ? s_val[tid - 1] : 0.f;
    const size_t obase = (size_t)w * (size_t)(MP + 1);
    for (int t = lag_lo; t <= lag_hi; ++t) {
      const float dv = dl[t];
      run += dv;
      const float c = dv / (run / (float)t + FLT_MIN);
      if (d_out) d_out[obase + t] = dv;
      if (c_out) c_out[obase + t] = c;
      dl[t] = c;
    }
    if (tid == 0) {
      if (d_out) d_out[obase] = 0.f;
      if (c_out) c_out[obase] = 1.f;
    }
    __syncthreads();

    // first trough under the threshold, and the minimum with the lowest index
    const float* y = dl + p.min_period;
    const int ny = MP - p.min_period + 1;                     // >= 3
    int first = INT_MAX, bi = INT_MAX;
    float bv = INFINITY;
    for (int i = tid; i < ny; i += T) {
      const float v = y[i];
      const bool trough = i == 0 ? v < y[1] : (i == ny - 1 ? false : (v < y[i - 1] && v <= y[i + 1]));
      if (trough && v < p.threshold && i < first) first = i;
      if (v < bv) bv = v, bi = i;
    }
    s_val[tid] = bv, s_idx[tid] = bi, s_first[tid] = first;
    __syncthreads();
    for (int off = T / 2; off > 0; off >>= 1) {
      if (tid < off) {
        const float v = s_val[tid + off];
        const int i = s_idx[tid + off];
        if (v < s_val[tid] || (v == s_val[tid] && i < s_idx[tid])) s_val[tid] = v, s_idx[tid] = i;
        s_first[tid] = min(s_first[tid], s_first[tid + off]);
      }
      __syncthreads();
    }
    if (tid == 0) {
      const bool is_voiced = s_first[0] != INT_MAX;
      int k = is_voiced ? s_first[0] : s_idx[0];
      if (k < 0 || k >= ny) k = 0;                            // no comparison held (NaN input): stay inside the range
      float shift = 0.f;
      if (k > 0 && k < ny - 1) {
        const float ym = y[k - 1], y0 = y[k], yp = y[k + 1];
        const float a = yp + ym - 2.f * y0, bb = (yp - ym) * 0.5f;
        if (fabsf(bb) < fabsf(a)) shift = -bb / a;
      }
      f0[w] = p.sr / ((float)(p.min_period + k) + shift);
      aperiodicity[w] = y[k];
      voiced[w] = is_voiced ? 1 : 0;
      if (index) index[w] = k;
    }
  }
}

// One block per row.  Terms in fp64; thread t adds frames t, t + 256, ... in order, then a tree over the threads.
__global__ void __launch_bounds__(256)
f0_compare_kernel(const float* __restrict__ f0_a, const uint8_t* __restrict__ voiced_a, const float* __restrict__ f0_b,
                  const uint8_t* __restrict__ voiced_b, int frames, double gross_cents, double* __restrict__ out) {
  const int tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * (size_t)frames;
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = tid; i < frames; i += 256) {
    const bool a = voiced_a[base + i] != 0, r = voiced_b[base + i] != 0;
    if (r) acc[0] += 1.0;
    if (a != r) acc[2] += 1.0;
    if (a && r) {
      const double cents = fabs(1200.0 * log2((double)f0_a[base + i] / (double)f0_b[base + i]));
      const bool gross = !(cents <= gross_cents);
      acc[1] += 1.0;
      acc[4] += cents;
      if (gross) acc[3] += 1.0;
      else acc[5] += cents;
    }
  }
  __shared__ double s[6][256];
#pragma unroll
  for (int q = 0; q < 6; ++q) s[q][tid] = acc[q];
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) {
#pragma unroll
      for (int q = 0; q < 6; ++q) s[q][tid] += s[q][tid + off];
    }
    __syncthreads();
  }
  if (tid < 6) out[(size_t)blockIdx.x * 6 + tid] = s[tid][0];
}

hipError_t yin_launch(const YinPlan& p, const float* x, int B, int64_t L, int frames, float* f0, float* aperiodicity,
                      uint8_t* voiced, int32_t* index, float* d, float* cmndf, hipStream_t s) {
  const int64_t work = (int64_t)B * frames;
  const int grid = (int)(work < (1 << 20) ? work : (1 << 20));
  yin_kernel<<<grid, PT_THREADS, yin_lds_bytes(p), s>>>(p, x, L, frames, work, f0, aperiodicity, voiced, index, d, cmndf);
  return hipGetLastError();
}

hipError_t f0_compare_launch(const float* f0_a, const uint8_t* voiced_a, const float* f0_b, const uint8_t* voiced_b, int B,
                             int frames, double gross_cents, double* out, hipStream_t s) {
  f0_compare_kernel<<<B, 256, 0, s>>>(f0_a, voiced_a, f0_b, voiced_b, frames, gross_cents, out);
  return hipGetLastError();
}
