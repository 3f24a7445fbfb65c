// F0-guided harmonic analysis, the additive harmonic template and the harmonic comparison; the definitions are in
// include/jat_hip_harm.h and, in fp64, in tests/harmonic_ref.py.  fp32 in both operand-dtype builds, no atomics.
//
// harm_analyze_kernel.  The harmonics of a frame lie between FFT bins and move from frame to frame, so every windowed frame is
// projected directly on exp(-i 2 pi h f0 n / sr).  One block takes one frame at a time: the windowed frame goes to LDS (the
// window's first half is made once per block, in fp64), and each of the four waves takes the harmonics h = 1 + wave, 5 + wave, ..
// Lane l adds the terms n = l, l + 64, .. in ascending n; the phase of a term is the uint32 product s n, kept as a running
// integer sum, so its angle never loses precision however long the frame.  The partial sums meet in a butterfly.  A harmonic
// that is not live costs nothing.  The loop is sincosf and two fmas a term: VALU work.
//
// harm_synth: three launches.  The phase of sample n is the sum of the increments before it, modulo 2^32, over up to millions
// of samples; in integers the sum is exact, so the scan may be split any way: a wave sums the increments of one frame, one
// block per row scans the frame sums, and the sample kernel scans inside the frame, 256 samples at a time, before it adds the
// harmonics in ascending order.
#include <math.h>

#include "jat_harmonic_kernels.h"

extern __shared__ __align__(16) float hm_lds[];

namespace {

constexpr double kPi = 3.14159265358979323846;
constexpr float kTurn = 1.4629180792671596e-9f;   // 2 pi 2^-32

__device__ inline bool hm_voiced(uint8_t flag, float f) { return flag != 0 && f > 0.f && isfinite(f); }

// f in [0, sr / 2): below 2^31
__device__ inline uint32_t hm_turns(double f, double sr) { return (uint32_t)llrint(f / sr * 4294967296.0); }

__device__ inline float hm_angle(uint32_t p) { return (float)(int32_t)p * kTurn; }

__device__ inline float hm_wave_sum(float v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, HM_WAVE);
  return v;
}

// the track at u in [0, 1) between two frames, in fp64 and without contraction: the increments must be numpy's
__device__ inline double hm_f0_at(float f0a, bool va, float f0b, bool vb, double u) {
#pragma clang fp contract(off)
  if (va && vb) {
    const double l = (1.0 - u) * (double)f0a, r = u * (double)f0b;
    return l + r;
  }
  return va ? (double)f0a : (vb ? (double)f0b : 0.0);
}

__device__ inline uint32_t hm_inc(const HarmPlan& p, double f0n) { return f0n < p.limit ? hm_turns(f0n, p.sr) : 0u; }

}  // namespace

__global__ void __launch_bounds__(HM_THREADS)
harm_analyze_kernel(HarmPlan p, const float* __restrict__ x, int64_t L, const float* __restrict__ f0,
                    const uint8_t* __restrict__ voiced, int frames, int64_t work, float* __restrict__ amp,
                    float* __restrict__ energy) {
  constexpr int T = HM_THREADS;
  const int tid = threadIdx.x, lane = tid & (HM_WAVE - 1), wave = tid / HM_WAVE;
  const int N = p.N, H = p.H, half = N / 2;
  float* xs = hm_lds;        // [N] the windowed frame
  float* wh = hm_lds + N;    // [N / 2 + 1] w[0 .. N / 2]; w[n] = w[N - n] behind it
  for (int i = tid; i <= half; i += T) wh[i] = (float)(0.5 - 0.5 * cos(2.0 * kPi * i / N));

  for (int64_t w = blockIdx.x; w < work; w += gridDim.x) {
    const int64_t b = w / frames;
    const int f = (int)(w - b * frames);
    const float* row = x + (size_t)b * (size_t)L;
    const int64_t first_sample = (int64_t)f * p.hop - half;
    __syncthreads();                                          // the window is made; the frame before is no longer read
    for (int i = tid; i < N; i += T) {
      const int64_t q = first_sample + i;
      xs[i] = (q >= 0 && q < L) ? wh[i <= half ? i : N - i] * row[q] : 0.f;
    }
    __syncthreads();

    if (energy && wave == 0) {
      float e = 0.f;
      for (int n = lane; n < N; n += HM_WAVE) e = fmaf(xs[n], xs[n], e);
      e = hm_wave_sum(e);
      if (lane == 0) energy[w] = e;
    }
    const float f0v = f0[w];
    const bool v = hm_voiced(voiced[w], f0v);
    for (int h = 1 + wave; h <= H; h += T / HM_WAVE) {
      const double hf = (double)h * (double)f0v;              // exact: 8 bits times 24
      float a = 0.f;
      if (v && hf < p.limit) {                                // the same for the whole wave
        const uint32_t s = hm_turns(hf, p.sr), step = s * (uint32_t)HM_WAVE;
        uint32_t ph = s * (uint32_t)lane;
        float re = 0.f, im = 0.f;
        for (int n = lane; n < N; n += HM_WAVE, ph += step) {
          float sn, cs;
          sincosf(hm_angle(ph), &sn, &cs);
          const float xv = xs[n];
          re = fmaf(xv, cs, re);
          im = fmaf(xv, sn, im);                              // the sign of the imaginary part does not reach |c|
        }
        re = hm_wave_sum(re), im = hm_wave_sum(im);
        a = 2.f * sqrtf(re * re + im * im) / (float)half;
      }
      if (lane == 0) amp[(size_t)w * (size_t)H + (size_t)(h - 1)] = a;
    }
  }
}

// work[b, f] = sum of inc[n] over the samples of frame f, one wave per frame
__global__ void __launch_bounds__(HM_THREADS)
harm_frame_sums_kernel(HarmPlan p, const float* __restrict__ f0, const uint8_t* __restrict__ voiced, int frames, int64_t L,
                       int64_t work, uint32_t* __restrict__ sums) {
  const int lane = threadIdx.x & (HM_WAVE - 1), wave = threadIdx.x / HM_WAVE;
  constexpr int WPB = HM_THREADS / HM_WAVE;
  for (int64_t w = (int64_t)blockIdx.x * WPB + wave; w < work; w += (int64_t)gridDim.x * WPB) {
    const int64_t b = w / frames;
    const int f = (int)(w - b * frames);
    const int64_t wb = b * frames + (f + 1 < frames ? f + 1 : frames - 1);
    const float f0a = f0[w], f0b = f0[wb];
    const bool va = hm_voiced(voiced[w], f0a), vb = hm_voiced(voiced[wb], f0b);
    const int64_t n0 = (int64_t)f * p.hop;
    const int64_t n1 = n0 + p.hop < L ? n0 + p.hop : L;
    uint32_t sum = 0;
    for (int64_t n = n0 + lane; n < n1; n += HM_WAVE)
      sum += hm_inc(p, hm_f0_at(f0a, va, f0b, vb, (double)(n - n0) / (double)p.hop));
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) sum += (uint32_t)__shfl_xor((int)sum, m, HM_WAVE);
    if (lane == 0) sums[w] = sum;
  }
}

// exclusive scan of a row's frame sums in place, modulo 2^32: one block per row, thread t owns a contiguous chunk
__global__ void __launch_bounds__(HM_THREADS)
harm_frame_scan_kernel(int frames, uint32_t* __restrict__ sums) {
  constexpr int T = HM_THREADS;
  const int tid = threadIdx.x;
  uint32_t* row = sums + (size_t)blockIdx.x * (size_t)frames;
  const int C = (frames + T - 1) / T;
  const int64_t lo = (int64_t)tid * C;
  const int64_t hi = lo + C < frames ? lo + C : frames;
  __shared__ uint32_t s[T];
  uint32_t part = 0;
  for (int64_t i = lo; i < hi; ++i) part += row[i];
  s[tid] = part;
  __syncthreads();
  for (int off = 1; off < T; off <<= 1) {
    const uint32_t v = tid >= off ? s[tid - off] : 0u;
    __syncthreads();
    s[tid] += v;
    __syncthreads();
  }
  uint32_t run = tid ? s[tid - 1] : 0u;
  for (int64_t i = lo; i < hi; ++i) {
    const uint32_t v = row[i];
    row[i] = run;
    run += v;
  }
}

__global__ void __launch_bounds__(HM_THREADS)
harm_synth_kernel(HarmPlan p, const float* __restrict__ f0, const uint8_t* __restrict__ voiced, const float* __restrict__ amp,
                  int frames, int64_t L, int64_t work, const uint32_t* __restrict__ base, float* __restrict__ y,
                  uint32_t* __restrict__ phase) {
  constexpr int T = HM_THREADS;
  const int tid = threadIdx.x, H = p.H;
  __shared__ float sa[2][T / 2];         // the amplitudes of frames f and f + 1, zero where the frame is unvoiced
  __shared__ uint32_t sc[T];
  static_assert(T / 2 >= 128, "one thread stages one harmonic");
  for (int64_t w = blockIdx.x; w < work; w += gridDim.x) {
    const int64_t b = w / frames;
    const int f = (int)(w - b * frames);
    const int64_t n0 = (int64_t)f * p.hop;
    const int64_t n1 = n0 + p.hop < L ? n0 + p.hop : L;
    if (n0 >= n1) continue;                                   // the last frame of a row whose length is a multiple of hop
    const int64_t wb = b * frames + (f + 1 < frames ? f + 1 : frames - 1);
    const float f0a = f0[w], f0b = f0[wb];
    const bool va = hm_voiced(voiced[w], f0a), vb = hm_voiced(voiced[wb], f0b);
    __syncthreads();                                          // the frame before is no longer read
    if (tid < H) {
      sa[0][tid] = va ? amp[(size_t)w * (size_t)H + tid] : 0.f;
      sa[1][tid] = vb ? amp[(size_t)wb * (size_t)H + tid] : 0.f;
    }
    uint32_t carry = base[w];
    const size_t rowoff = (size_t)b * (size_t)L;
    for (int64_t t0 = n0; t0 < n1; t0 += T) {
      const int64_t n = t0 + tid;
      const bool active = n < n1;
      const double u = (double)(n - n0) / (double)p.hop;
      const double f0n = active ? hm_f0_at(f0a, va, f0b, vb, u) : 0.0;
      const uint32_t inc = active ? hm_inc(p, f0n) : 0u;
      sc[tid] = inc;
      __syncthreads();                                        // also: sa is staged
      for (int off = 1; off < T; off <<= 1) {
        const uint32_t v = tid >= off ? sc[tid - off] : 0u;
        __syncthreads();
        sc[tid] += v;
        __syncthreads();
      }
      const uint32_t ph = carry + (sc[tid] - inc);
      carry += sc[T - 1];
      if (active) {
        if (phase) phase[rowoff + (size_t)n] = ph;
        const float uf = (float)u, lf = 1.f - uf;
        float acc = 0.f;
        if (f0n > 0.0) {
          for (int h = 1; h <= H; ++h) {
            if (!((double)h * f0n < p.limit)) break;          // at or above Nyquist, and so is every later one
            const float a = lf * sa[0][h - 1] + uf * sa[1][h - 1];
            acc = fmaf(a, sinf(hm_angle((uint32_t)h * ph)), acc);
          }
        }
        y[rowoff + (size_t)n] = acc;
      }
      __syncthreads();                                        // sc is read before the next tile overwrites it
    }
  }
}

// One block per row.  Terms in fp64; thread t adds the cells t, t + 256, .. in order, then a tree over the threads.
__global__ void __launch_bounds__(HM_THREADS)
harm_compare_kernel(const float* __restrict__ amp_a, const float* __restrict__ amp_ref, const float* __restrict__ f0_ref,
                    const uint8_t* __restrict__ voiced_ref, int frames, int H, double cutoff_hz, double floor_,
                    double* __restrict__ out) {
  constexpr int T = HM_THREADS;
  const int tid = threadIdx.x;
  const size_t fbase = (size_t)blockIdx.x * (size_t)frames;
  const int64_t cells = (int64_t)frames * H;
  double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t i = tid; i < cells; i += T) {
    const int64_t f = i / H;
    const int h = (int)(i - f * H) + 1;
    const float fr = f0_ref[fbase + f];
    const float ar = amp_ref[fbase * H + i];
    if (!hm_voiced(voiced_ref[fbase + f], fr) || !((double)ar > floor_)) continue;
    const double e = 20.0 * log10(((double)amp_a[fbase * H + i] + floor_) / ((double)ar + floor_));
    const int o = (double)h * (double)fr < cutoff_hz ? 0 : 4;
    acc[o] += 1.0, acc[o + 1] += e, acc[o + 2] += e * e, acc[o + 3] += fabs(e);
  }
  __shared__ double s[8][T];
#pragma unroll
  for (int q = 0; q < 8; ++q) s[q][tid] = acc[q];
  __syncthreads();
  for (int off = T / 2; off > 0; off >>= 1) {
    if (tid < off) {
#pragma unroll
      for (int q = 0; q < 8; ++q) s[q][tid] += s[q][tid + off];
    }
    __syncthreads();
  }
  if (tid < 8) out[(size_t)blockIdx.x * 8 + tid] = s[tid][0];
}

static int harm_grid(int64_t blocks, int64_t cap) { return (int)(blocks < cap ? blocks : cap); }

hipError_t harm_analyze_launch(const HarmPlan& p, const float* x, int B, int64_t L, const float* f0, const uint8_t* voiced,
                               int frames, float* amp, float* energy, hipStream_t s) {
  const int64_t work = (int64_t)B * frames;
  harm_analyze_kernel<<<harm_grid(work, 2048), HM_THREADS, harm_analyze_lds_bytes(p), s>>>(p, x, L, f0, voiced, frames, work,
                                                                                           amp, energy);
  return hipGetLastError();
}

hipError_t harm_synth_launch(const HarmPlan& p, const float* f0, const uint8_t* voiced, const float* amp, int B, int frames,
                             int64_t L, float* y, uint32_t* phase, uint32_t* work_buf, hipStream_t s) {
  const int64_t work = (int64_t)B * frames;
  constexpr int WPB = HM_THREADS / HM_WAVE;
  harm_frame_sums_kernel<<<harm_grid((work + WPB - 1) / WPB, 1 << 16), HM_THREADS, 0, s>>>(p, f0, voiced, frames, L, work,
                                                                                           work_buf);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  harm_frame_scan_kernel<<<B, HM_THREADS, 0, s>>>(frames, work_buf);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  harm_synth_kernel<<<harm_grid(work, 1 << 20), HM_THREADS, 0, s>>>(p, f0, voiced, amp, frames, L, work, work_buf, y, phase);
  return hipGetLastError();
}

hipError_t harm_compare_launch(const float* amp_a, const float* amp_ref, const float* f0_ref, const uint8_t* voiced_ref, int B,
                               int frames, int H, double cutoff_hz, double floor_, double* out, hipStream_t s) {
  harm_compare_kernel<<<B, HM_THREADS, 0, s>>>(amp_a, amp_ref, f0_ref, voiced_ref, frames, H, cutoff_hz, floor_, out);
  return hipGetLastError();
}
