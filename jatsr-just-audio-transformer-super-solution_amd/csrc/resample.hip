// Polyphase windowed-sinc sample-rate converter (torchaudio functional.resample, sinc_interp_hann) and the per-channel
// fp64 statistics of fp16-rounded latents.  Plain fp32 VALU + LDS: 47.6 s of audio is 0.7 GFLOP against 17 MB of traffic.
//
// Resampler: output frame f holds the n outputs y[f n + p] = sum_k h[p][k] x[f o + k - width].  A block takes a run of
// frames of one batch row and one slice of the phases.  It stages the run's input window (zero outside [0, L)) into LDS once
// with coalesced loads.  A thread owns PH phases and RS_FRAMES frames: per tap it loads its PH table entries (the table is
// stored [K][n], so the lanes of a wave read consecutive words) and RS_FRAMES window samples (the lanes of one frame group
// read the same LDS word: a broadcast), and does PH * RS_FRAMES FMAs, so a table row is read once per block and frame group,
// not once per output; the table loads run one tile of taps ahead of their use.  Every output is one thread's sum over k in
// ascending order whatever the batch or the block it falls in: results are bit-identical from run to run and between a row
// run alone and in a batch.  No atomics.
#include <hip/hip_fp16.h>

#include "jat_resample_kernels.h"

namespace {

template <int PH>
__global__ void __launch_bounds__(RS_MAX_THREADS)
resample_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ ht, int L, int L_out,
                int n_frames, int o, int n, int width, int K, int pn, int lanes, int groups) {
  constexpr int R = RS_FRAMES;
  extern __shared__ float xs[];
  const int tid = threadIdx.x;
  const int fb = blockIdx.x * groups * R;
  const int nfr = min(groups * R, n_frames - fb);
  const float* xr = x + (int64_t)blockIdx.z * L;
  float* yr = y + (int64_t)blockIdx.z * L_out;

  const int W = (nfr - 1) * o + K;
  const int64_t start = (int64_t)fb * o - width;
  // eight loads in flight per thread: one wait per eight samples instead of one per sample
  for (int i0 = tid; i0 < W; i0 += 8 * blockDim.x) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = i0 + u * blockDim.x;
      const int64_t g = start + i;
      v[u] = (i < W && g >= 0 && g < L) ? xr[g] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = i0 + u * blockDim.x;
      if (i < W) xs[i] = v[u];
    }
  }
  __syncthreads();

  const int j = tid / lanes, l = tid - j * lanes;
  const int pbase = blockIdx.y * pn;
  int pc[PH];        // table column, clamped so that the loads of an idle slot stay inside the table
  bool pv[PH];
#pragma unroll
  for (int i = 0; i < PH; ++i) {
    const int q = l + i * lanes;
    pv[i] = q < pn && pbase + q < n;
    pc[i] = pv[i] ? pbase + q : n - 1;
  }
  int xo[R];         // window offset of frame r * groups + j (an idle slot reads frame 0 and is not written)
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int f = r * groups + j;
    xo[r] = f < nfr ? f * o : 0;
  }
  float acc[PH][R];
#pragma unroll
  for (int i = 0; i < PH; ++i)
#pragma unroll
    for (int r = 0; r < R; ++r) acc[i][r] = 0.f;

  // Taps in tiles of U: the table entries of the next tile are in flight while the current one is used, so the latency of
  // the table loads (L2) is paid once, not once per tap.  Every output still adds its products in ascending k.
  constexpr int U = RS_TAP_TILE;
  const int k_tiles = K / U * U;
  float hn[U][PH];
  if (k_tiles > 0) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int i = 0; i < PH; ++i) hn[u][i] = ht[(size_t)u * n + pc[i]];
  }
  for (int k0 = 0; k0 < k_tiles; k0 += U) {
    float hc[U][PH];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int i = 0; i < PH; ++i) hc[u][i] = hn[u][i];
    if (k0 + U < k_tiles) {
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int i = 0; i < PH; ++i) hn[u][i] = ht[(size_t)(k0 + U + u) * n + pc[i]];
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float* xp = xs + xo[r] + k0;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float xv = xp[u];
#pragma unroll
        for (int i = 0; i < PH; ++i) acc[i][r] = fmaf(hc[u][i], xv, acc[i][r]);
      }
    }
  }
  for (int k = k_tiles; k < K; ++k) {
    float h[PH];
#pragma unroll
    for (int i = 0; i < PH; ++i) h[i] = ht[(size_t)k * n + pc[i]];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float xv = xs[xo[r] + k];
#pragma unroll
      for (int i = 0; i < PH; ++i) acc[i][r] = fmaf(h[i], xv, acc[i][r]);
    }
  }

#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int f = r * groups + j;
    if (f >= nfr) continue;
#pragma unroll
    for (int i = 0; i < PH; ++i) {
      const int64_t idx = (int64_t)(fb + f) * n + pc[i];
      if (pv[i] && idx < L_out) yr[idx] = acc[i][r];
    }
  }
}

// Stage 1: block (c, s) sums slice s of the B * T values of channel c; thread-strided partial sums, then a fixed tree.
__global__ void __launch_bounds__(256)
stats_partial_kernel(const float* __restrict__ z, int C, int T, int64_t BT, double* __restrict__ partial) {
  __shared__ double s1[256], s2[256];
  const int c = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
  const int64_t chunk = (BT + STATS_SLICES - 1) / STATS_SLICES;
  const int64_t i0 = (int64_t)s * chunk, i1 = min(BT, i0 + chunk);
  double a = 0.0, q = 0.0;
  for (int64_t i = i0 + tid; i < i1; i += 256) {
    const int64_t b = i / T, t = i - b * T;
    const double v = (double)__half2float(__float2half_rn(z[(b * C + c) * T + t]));
    a += v;
    q += v * v;
  }
  s1[tid] = a;
  s2[tid] = q;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) {
      s1[tid] += s1[tid + w];
      s2[tid] += s2[tid + w];
    }
    __syncthreads();
  }
  if (tid == 0) {
    partial[((size_t)c * STATS_SLICES + s) * 2] = s1[0];
    partial[((size_t)c * STATS_SLICES + s) * 2 + 1] = s2[0];
  }
}

// Stage 2: one thread per channel adds its slices in order and folds them into the caller's running totals.
__global__ void __launch_bounds__(256)
stats_finish_kernel(const double* __restrict__ partial, int C, double* __restrict__ sum, double* __restrict__ sq) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  double a = 0.0, q = 0.0;
  for (int s = 0; s < STATS_SLICES; ++s) {
    a += partial[((size_t)c * STATS_SLICES + s) * 2];
    q += partial[((size_t)c * STATS_SLICES + s) * 2 + 1];
  }
  sum[c] += a;
  sq[c] += q;
}

}  // namespace

bool resample_geometry(int o, int n, int K, ResampleGeom* g) {
  g->ph = n >= 32 ? 4 : 1;
  const int cap = RS_MAX_THREADS * g->ph;            // phases one block can hold
  g->slices = (n + cap - 1) / cap;
  g->pn = (n + g->slices - 1) / g->slices;
  g->slices = (n + g->pn - 1) / g->pn;
  g->lanes = (g->pn + g->ph - 1) / g->ph;
  g->groups = RS_MAX_THREADS / g->lanes;
  while (g->groups > 1 && ((int64_t)g->groups * RS_FRAMES - 1) * o + K > RS_MAX_WINDOW) --g->groups;
  return ((int64_t)g->groups * RS_FRAMES - 1) * o + K <= RS_MAX_WINDOW;
}

// Frame groups for one launch: few enough that a clip of some seconds still gives every CU a few blocks, and a thread count
// that leaves at most 15 % of the last wave idle where such a count exists.  The result of an output does not depend on it.
static int pick_groups(const ResampleGeom& g, int n_frames) {
  int want = n_frames / (RS_FRAMES * 768);
  want = want < 1 ? 1 : (want > g.groups ? g.groups : want);
  for (int c = want; c <= g.groups; ++c) {
    const int t = g.lanes * c, waves = (t + 63) / 64;
    if (t * 100 >= waves * 64 * 85) return c;
  }
  return want;
}

ResampleLaunch resample_launch_shape(const ResampleGeom& g, int L_out, int o, int n, int K) {
  ResampleLaunch a;
  a.n_frames = (int)(((int64_t)L_out + n - 1) / n);
  a.groups = pick_groups(g, a.n_frames);
  a.fpb = a.groups * RS_FRAMES;
  a.grid_x = (unsigned)((a.n_frames + a.fpb - 1) / a.fpb);
  a.block = g.lanes * a.groups;
  a.lds = ((size_t)(a.fpb - 1) * o + K) * sizeof(float);
  return a;
}

hipError_t resample_launch(const float* x, float* y, const float* ht, int B, int L, int L_out, int o, int n, int width, int K,
                           const ResampleGeom& g, hipStream_t s) {
  const ResampleLaunch a = resample_launch_shape(g, L_out, o, n, K);
  const dim3 grid(a.grid_x, g.slices, B), block(a.block);
  if (g.ph == 4)
    resample_kernel<4><<<grid, block, a.lds, s>>>(x, y, ht, L, L_out, a.n_frames, o, n, width, K, g.pn, g.lanes, a.groups);
  else
    resample_kernel<1><<<grid, block, a.lds, s>>>(x, y, ht, L, L_out, a.n_frames, o, n, width, K, g.pn, g.lanes, a.groups);
  return hipGetLastError();
}

hipError_t channel_stats_launch(const float* z, int B, int C, int T, double* partial, double* sum, double* sq, hipStream_t s) {
  stats_partial_kernel<<<dim3(C, STATS_SLICES), 256, 0, s>>>(z, C, T, (int64_t)B * T, partial);
  stats_finish_kernel<<<(C + 255) / 256, 256, 0, s>>>(partial, C, sum, sq);
  return hipGetLastError();
}
