// Inverse STFT, low-band splice and long-term average spectrum on the transform of metrics.hip (jat_fft.h): plain fp32
// VALU + LDS, no atomics, the same code in both operand-dtype builds.  Definitions in include/jat_hip.h.
//
// Two real frames share one complex transform end to end.  Forward: z = u + i v.  A real, symmetric gain a[N - k] = a[k]
// keeps the two apart, ifft(a fft(u + i v)) = irfft(a rfft(u)) + i irfft(a rfft(v)), so the splice needs no split step; the
// inverse STFT packs Z = Xa + i Xb with the Hermitian halves written out (the imaginary parts of the DC and Nyquist bins are
// dropped, as irfft drops them).  The inverse runs through the forward passes and twiddles: ifft(Z) = conj(fft(conj Z)) / N;
// 1 / N is a power of two, so the scaling is exact.  Frames pair as (2 p, 2 p + 1) whatever the batch or the block cut.
//
// Overlap-add: the transform kernels write the windowed frames w[i] y_f[i] to a workspace [B, frames, N]; a gather pass
// then forms every output sample as the sum of its n_fft / hop covering frames in ascending frame order, divides by the
// host-made envelope (jat_splice_kernels.h) and, for the splice, adds the generated sample.  The order is fixed per sample,
// so the result has the same bits from run to run, for a row alone or in a batch, and whatever the block cut.
//
// Long-term spectrum: frames (2 p, 2 p + 1) ride one transform, are split as in metrics.hip, and a thread adds the powers
// of its bins in fp64 over the frames of its slice in ascending order; LT_SLICES partial spectra per row (a cut that does
// not depend on the batch), then one thread per bin adds the slices in order.  No spectrogram reaches memory.
#include "jat_fft.h"
#include "jat_splice_kernels.h"

namespace {

struct SpliceLds {
  float2 *buf0, *buf1, *tw;
  float* gain;
};
__device__ __forceinline__ SpliceLds splice_lds(const MetricsPlan& p, float2* lds) {
  SpliceLds s;
  s.buf0 = lds;
  s.buf1 = lds + p.group * p.n_fft;
  s.tw = s.buf1 + p.group * p.n_fft;
  s.gain = (float*)(s.tw + ((p.n_tw + 1) & ~1));   // [bins]
  return s;
}

// The spectra of conj Z after pass 0 lie in b0 (a barrier behind them): the remaining passes, then frame 2 (pair0 + g) takes
// w Re / N and frame 2 (pair0 + g) + 1 takes -w Im / N (the conjugate of the result), to Wrow [frames, N].  Ends on a barrier.
__device__ __forceinline__ void inverse_tail(const MetricsPlan& p, const MetricsTables& t, const float2* tw, float2* b0,
                                             float2* b1, int tid, int pair0, int frames, float* __restrict__ Wrow) {
  const int N = p.n_fft, G = p.group, lN = 31 - __clz(N);
  float2* other;
  const float2* R = fft_later_passes(p, tw, b0, b1, G, tid, &other);
  const float inv = 1.f / (float)N;
  for (int jj = tid; jj < G * N; jj += MT_THREADS) {
    const int g = jj >> lN, i = jj & (N - 1), f0 = 2 * (pair0 + g);
    if (f0 < frames) {
      const float2 r = R[g * N + i];
      const float w = t.window[i] * inv;
      Wrow[(int64_t)f0 * N + i] = w * r.x;
      if (f0 + 1 < frames) Wrow[(int64_t)(f0 + 1) * N + i] = w * -r.y;
    }
  }
  __syncthreads();                           // the next group overwrites both buffers
}

__global__ void __launch_bounds__(MT_THREADS)
istft_frames_kernel(MetricsPlan p, MetricsTables t, const float2* __restrict__ X, int frames, int gpb, float* __restrict__ W) {
  extern __shared__ __align__(16) float2 lds[];
  const SpliceLds m = splice_lds(p, lds);
  const int N = p.n_fft, G = p.group, bins = p.bins, tid = threadIdx.x, b = blockIdx.y;
  for (int i = tid; i < p.n_tw; i += MT_THREADS) m.tw[i] = t.tw[i];
  __syncthreads();
  const float2* Xr = X + (int64_t)b * bins * frames;
  float* Wrow = W + (int64_t)b * frames * N;
  const int q = N >> 2, lq = 31 - __clz(q), h = N >> 1;
  for (int grp = 0; grp < gpb; ++grp) {
    const int pair0 = (blockIdx.x * gpb + grp) * G;
    if (2 * pair0 >= frames) break;          // the same for every thread of the block
    // pass 0 on conj Z, Z[k] = Xa[k] + i Xb[k] for k <= N / 2 and conj Xa[N - k] + i conj Xb[N - k] above
    for (int jj = tid; jj < G * q; jj += MT_THREADS) {
      const int g = jj >> lq, j = jj & (q - 1), f0 = 2 * (pair0 + g);
      float2 v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = j + r * q, k = i <= h ? i : N - i;
        float2 xa = make_float2(0.f, 0.f), xb = xa;
        if (f0 < frames) xa = Xr[(int64_t)k * frames + f0];
        if (f0 + 1 < frames) xb = Xr[(int64_t)k * frames + f0 + 1];
        if (k == 0 || k == h) xa.y = 0.f, xb.y = 0.f;
        if (i > h) xa.y = -xa.y, xb.y = -xb.y;
        v[r] = make_float2(xa.x - xb.y, -(xa.y + xb.x));
      }
      fft_first_pass(v, m.buf0 + g * N, j);
    }
    __syncthreads();
    inverse_tail(p, t, m.tw, m.buf0, m.buf1, tid, pair0, frames, Wrow);
  }
}

__global__ void __launch_bounds__(MT_THREADS)
splice_frames_kernel(MetricsPlan p, MetricsTables t, const float* __restrict__ gen, const float* __restrict__ src,
                     int64_t L_gen, int64_t L_src, int n, int frames, int gpb, const float* __restrict__ gain,
                     float* __restrict__ W) {
  extern __shared__ __align__(16) float2 lds[];
  const SpliceLds m = splice_lds(p, lds);
  const int N = p.n_fft, G = p.group, bins = p.bins, tid = threadIdx.x, b = blockIdx.y;
  for (int i = tid; i < p.n_tw; i += MT_THREADS) m.tw[i] = t.tw[i];
  for (int i = tid; i < bins; i += MT_THREADS) m.gain[i] = gain[i];
  __syncthreads();
  const float* gr = gen + (int64_t)b * L_gen;
  const float* sr = src + (int64_t)b * L_src;
  float* Wrow = W + (int64_t)b * frames * N;
  const int q = N >> 2, lq = 31 - __clz(q), h = N >> 1;
  for (int grp = 0; grp < gpb; ++grp) {
    const int pair0 = (blockIdx.x * gpb + grp) * G;
    if (2 * pair0 >= frames) break;          // the same for every thread of the block
    // forward pass 0 on w (src - gen) of frames 2 p (real part) and 2 p + 1 (imaginary part), zeros outside [0, n)
    for (int jj = tid; jj < G * q; jj += MT_THREADS) {
      const int g = jj >> lq, j = jj & (q - 1), f0 = 2 * (pair0 + g);
      float2 v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = j + r * q;
        const int64_t s0 = (int64_t)f0 * p.hop + i - h, s1 = s0 + p.hop;
        const bool in0 = f0 < frames && s0 >= 0 && s0 < n, in1 = f0 + 1 < frames && s1 >= 0 && s1 < n;
        const float w = t.window[i];
        v[r] = make_float2(in0 ? w * (sr[s0] - gr[s0]) : 0.f, in1 ? w * (sr[s1] - gr[s1]) : 0.f);
      }
      fft_first_pass(v, m.buf0 + g * N, j);
    }
    __syncthreads();
    float2* free_buf;
    float2* Z = fft_later_passes(p, m.tw, m.buf0, m.buf1, G, tid, &free_buf);
    // inverse pass 0 on conj(a Z), the gain applied symmetrically
    for (int jj = tid; jj < G * q; jj += MT_THREADS) {
      const int g = jj >> lq, j = jj & (q - 1);
      float2 v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = j + r * q;
        const float a = m.gain[i <= h ? i : N - i];
        const float2 z = Z[g * N + i];
        v[r] = make_float2(a * z.x, -(a * z.y));
      }
      fft_first_pass(v, free_buf + g * N, j);
    }
    __syncthreads();
    inverse_tail(p, t, m.tw, free_buf, Z, tid, pair0, frames, Wrow);
  }
}

__global__ void __launch_bounds__(256)
overlap_add_kernel(int N, int hop, const float* __restrict__ W, const float* __restrict__ envelope, int frames, int n,
                   const float* __restrict__ gen, int64_t L_out, float* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (t >= L_out) return;
  if (t >= n) {                              // past the shorter signal: only reached with gen
    out[b * L_out + t] = gen[b * L_out + t];
    return;
  }
  const int R = N / hop, pos = (int)t + (N >> 1), q = pos / hop, r = pos - q * hop;
  const int m_hi = q < R - 1 ? q : R - 1, m_lo = q - (frames - 1) > 0 ? q - (frames - 1) : 0;
  const float* Wrow = W + (int64_t)b * frames * N;
  float acc = 0.f;
  for (int m = m_hi; m >= m_lo; --m) acc += Wrow[(int64_t)(q - m) * N + r + m * hop];   // frames q - m ascending
  const float y = acc / envelope[(m_hi * (m_hi + 1) / 2 + m_lo) * hop + r];
  if (gen) {
    const float g = gen[b * L_out + t];
    out[b * L_out + t] = acc == 0.f ? g : g + y;   // a zero correction leaves the sample's bits (its sign of zero too)
  } else {
    out[b * L_out + t] = y;
  }
}

__global__ void __launch_bounds__(MT_THREADS)
ltas_partial_kernel(MetricsPlan p, MetricsTables t, const float* __restrict__ x, int L, int frames, int chunk,
                    double* __restrict__ partial) {
  extern __shared__ __align__(16) float2 lds[];
  const SpliceLds m = splice_lds(p, lds);
  const int N = p.n_fft, G = p.group, bins = p.bins, tid = threadIdx.x, s = blockIdx.x, b = blockIdx.y;
  for (int i = tid; i < p.n_tw; i += MT_THREADS) m.tw[i] = t.tw[i];
  __syncthreads();
  const float* xr = x + (int64_t)b * L;
  const int q = N >> 2, lq = 31 - __clz(q), h = N >> 1;
  const int pairs = (frames + 1) >> 1, pend = min(pairs, (s + 1) * chunk);
  double acc[LT_BINS_PER_THREAD];
#pragma unroll
  for (int u = 0; u < LT_BINS_PER_THREAD; ++u) acc[u] = 0.0;
  for (int pair0 = s * chunk; pair0 < pend; pair0 += G) {
    for (int jj = tid; jj < G * q; jj += MT_THREADS) {
      const int g = jj >> lq, j = jj & (q - 1), f0 = 2 * (pair0 + g);
      const bool mine = pair0 + g < pend;    // a group may reach past the slice: those frames belong to the next block
      float2 v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = j + r * q;
        const int64_t s0 = (int64_t)f0 * p.hop + i - h, s1 = s0 + p.hop;
        const bool in0 = mine && f0 < frames && s0 >= 0 && s0 < L, in1 = mine && f0 + 1 < frames && s1 >= 0 && s1 < L;
        const float w = t.window[i];
        v[r] = make_float2(in0 ? w * xr[s0] : 0.f, in1 ? w * xr[s1] : 0.f);
      }
      fft_first_pass(v, m.buf0 + g * N, j);
    }
    __syncthreads();
    float2* free_buf;
    const float2* Z = fft_later_passes(p, m.tw, m.buf0, m.buf1, G, tid, &free_buf);
    for (int g = 0; g < G && pair0 + g < pend; ++g) {
      const int f0 = 2 * (pair0 + g);
#pragma unroll
      for (int u = 0; u < LT_BINS_PER_THREAD; ++u) {
        const int k = tid + u * MT_THREADS;
        if (k < bins) {
          const float2 a = Z[g * N + k], c = Z[g * N + ((N - k) & (N - 1))];
          const double ar = 0.5f * (a.x + c.x), ai = 0.5f * (a.y - c.y);      // frame f0
          const double br = 0.5f * (a.y + c.y), bi = -0.5f * (a.x - c.x);     // frame f0 + 1
          if (f0 < frames) acc[u] += ar * ar + ai * ai;
          if (f0 + 1 < frames) acc[u] += br * br + bi * bi;
        }
      }
    }
    __syncthreads();                         // the next group overwrites both buffers
  }
  double* o = partial + ((int64_t)b * LT_SLICES + s) * bins;
#pragma unroll
  for (int u = 0; u < LT_BINS_PER_THREAD; ++u) {
    const int k = tid + u * MT_THREADS;
    if (k < bins) o[k] = acc[u];
  }
}

__global__ void __launch_bounds__(256)
ltas_final_kernel(const double* __restrict__ partial, int bins, int frames, double* __restrict__ P) {
  const int k = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (k >= bins) return;
  double sum = 0.0;
  for (int s = 0; s < LT_SLICES; ++s) sum += partial[((int64_t)b * LT_SLICES + s) * bins + k];
  P[(int64_t)b * bins + k] = sum / (double)frames;
}

template <typename K>
hipError_t allow_lds(K kernel, size_t lds) {
  if (lds <= 64 * 1024) return hipSuccess;
  return hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

// groups of p.group frame pairs a block runs through: as few as keep the launch within one round of blocks
void frames_grid(const MetricsPlan& p, int slots, int B, int frames, int* gpb, dim3* grid) {
  const int pairs = (frames + 1) / 2, groups = (pairs + p.group - 1) / p.group;
  int64_t g = ((int64_t)groups * B + slots - 1) / slots;
  *gpb = (int)(g < 1 ? 1 : (g > 64 ? 64 : g));
  *grid = dim3((groups + *gpb - 1) / *gpb, B);
}

}  // namespace

size_t splice_lds_bytes(const MetricsPlan& p) {
  return ((size_t)2 * p.group * p.n_fft + ((p.n_tw + 1) & ~1)) * sizeof(float2) + (size_t)((p.bins + 3) & ~3) * sizeof(float);
}

hipError_t splice_blocks_per_cu(const MetricsPlan& p, int* blocks) {
  const size_t lds = splice_lds_bytes(p);
  hipError_t e = allow_lds(splice_frames_kernel, lds);
  if (e != hipSuccess) return e;
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, (const void*)splice_frames_kernel, MT_THREADS, lds);
}

hipError_t istft_frames_launch(const MetricsPlan& p, const MetricsTables& t, int slots, const float2* X, int B, int frames,
                               float* W, hipStream_t s) {
  const size_t lds = splice_lds_bytes(p);
  hipError_t e = allow_lds(istft_frames_kernel, lds);
  if (e != hipSuccess) return e;
  int gpb;
  dim3 grid;
  frames_grid(p, slots, B, frames, &gpb, &grid);
  istft_frames_kernel<<<grid, MT_THREADS, lds, s>>>(p, t, X, frames, gpb, W);
  return hipGetLastError();
}

hipError_t splice_frames_launch(const MetricsPlan& p, const MetricsTables& t, int slots, const float* gen, const float* src,
                                int B, int64_t L_gen, int64_t L_src, int n, int frames, const float* gain, float* W,
                                hipStream_t s) {
  const size_t lds = splice_lds_bytes(p);
  hipError_t e = allow_lds(splice_frames_kernel, lds);
  if (e != hipSuccess) return e;
  int gpb;
  dim3 grid;
  frames_grid(p, slots, B, frames, &gpb, &grid);
  splice_frames_kernel<<<grid, MT_THREADS, lds, s>>>(p, t, gen, src, L_gen, L_src, n, frames, gpb, gain, W);
  return hipGetLastError();
}

hipError_t overlap_add_launch(const MetricsPlan& p, const float* W, const float* envelope, int B, int frames, int n,
                              const float* gen, int64_t L_out, float* out, hipStream_t s) {
  const dim3 grid((unsigned)((L_out + 255) / 256), B);
  overlap_add_kernel<<<grid, 256, 0, s>>>(p.n_fft, p.hop, W, envelope, frames, n, gen, L_out, out);
  return hipGetLastError();
}

hipError_t ltas_launch(const MetricsPlan& p, const MetricsTables& t, const float* x, int B, int L, int frames, double* partial,
                       double* P, hipStream_t s) {
  const size_t lds = splice_lds_bytes(p);
  hipError_t e = allow_lds(ltas_partial_kernel, lds);
  if (e != hipSuccess) return e;
  const int pairs = (frames + 1) / 2, chunk = (pairs + LT_SLICES - 1) / LT_SLICES;
  ltas_partial_kernel<<<dim3(LT_SLICES, B), MT_THREADS, lds, s>>>(p, t, x, L, frames, chunk, partial);
  ltas_final_kernel<<<dim3((p.bins + 255) / 256, B), 256, 0, s>>>(partial, p.bins, frames, P);
  return hipGetLastError();
}
