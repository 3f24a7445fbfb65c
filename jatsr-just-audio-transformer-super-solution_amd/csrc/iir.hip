// IIR low-pass cascades (include/jat_hip_iir.h): up to five direct-form-II-transposed second-order sections per
// row as an exact blocked linear recurrence.  A lane owns IIR_LANE_BLOCK consecutive samples, a workgroup a tile of IIR_TILE.
//   pass A  iir_tile_kernel<false>: every lane runs its block from zero state, the workgroup scans the affine maps s -> P s + e
//           (P = A^IIR_LANE_BLOCK, Hillis-Steele over the precomputed powers P^(2^k)) and writes the state behind its tile;
//   pass B  iir_carry_kernel: one wave per row carries the tile states along the row with A^IIR_TILE from the row's seed;
//   pass C  iir_tile_kernel<true>: the same scan with lane 0 started from the tile's true start state, then every lane re-runs
//           its block from its true start state and the tile is written.
// The launches are the only synchronisation between workgroups.  Every product and sum is rounded once (contraction is off for
// this file), in the order tests/lowpass_ref.py states in numpy, so the twin there gives these bits.
#include <hip/hip_runtime.h>

#include "jat_iir_kernels.h"

#pragma clang fp contract(off)

namespace {

// sample p of a row in processing order (header: IirMode); src is the row
__device__ __forceinline__ float iir_load(const float* src, int mode, int n, int pl, int m, int p) {
  if (mode == IIR_PLAIN) return src[p];
  if (mode == IIR_BACKWARD) return src[m - 1 - p];
  if (p < pl) return 2.f * src[0] - src[pl - p];
  if (p < pl + n) return src[p - pl];
  return 2.f * src[n - 1] - src[n - 2 - (p - pl - n)];
}

// one sample through the filter's own sections; identity padding is skipped (nsec is the same in every lane)
__device__ __forceinline__ float iir_step(const IirFilter& F, int nsec, float (&s)[IIR_STATE], float x) {
#pragma unroll
  for (int k = 0; k < IIR_SECTIONS; ++k) {
    if (k < nsec) {
      const float y = F.c[k][0] * x + s[2 * k];
      s[2 * k] = (F.c[k][1] * x - F.c[k][3] * y) + s[2 * k + 1];
      s[2 * k + 1] = F.c[k][2] * x - F.c[k][4] * y;
      x = y;
    }
  }
  return x;
}

__device__ __forceinline__ const IirFilter& iir_filter(const IirFilter* tab, int R, const int32_t* row_filter, int row) {
  const int f = __builtin_amdgcn_readfirstlane(min(max(row_filter[row], 0), R - 1));   // clamped: never a wild read
  return tab[f];
}

template <bool WRITE>
__global__ __launch_bounds__(IIR_THREADS) void iir_tile_kernel(const IirFilter* __restrict__ tab, int R,
                                                               const int32_t* __restrict__ row_filter, const float* src,
                                                               float* dst, float* states, int n, int nt, int mode) {
  // a lane reads its block at stride 33: banks (lane + i) mod 32, conflict-free in both halves of the wave
  __shared__ float xs[IIR_TILE + IIR_TILE / 32];
  __shared__ float es[IIR_STATE * IIR_THREADS];
  const int row = blockIdx.y, tile = blockIdx.x, lane = threadIdx.x;
  const IirFilter& F = iir_filter(tab, R, row_filter, row);
  const int nsec = F.nsec, pl = F.padlen;
  const int m = mode == IIR_PLAIN ? n : n + 2 * pl;
  const int t0 = tile * IIR_TILE;
  if (t0 >= m) return;                                     // the grid covers the longest extension
  const size_t ext = (size_t)n + 2 * IIR_MAX_PADLEN;
  const float* in = src + (size_t)row * (mode == IIR_BACKWARD ? ext : (size_t)n);
#pragma unroll 4
  for (int k = 0; k < IIR_LANE_BLOCK; ++k) {
    const int idx = k * IIR_THREADS + lane, p = t0 + idx;
    xs[idx + (idx >> 5)] = p < m ? iir_load(in, mode, n, pl, m, p) : 0.f;
  }
  __syncthreads();
  float* st = states + ((size_t)row * nt + tile) * IIR_STATE;
  float s[IIR_STATE], s0[IIR_STATE];
#pragma unroll
  for (int c = 0; c < IIR_STATE; ++c) s[c] = s0[c] = (WRITE && lane == 0) ? st[c] : 0.f;
  float* xl = xs + lane * (IIR_LANE_BLOCK + 1);
  for (int i = 0; i < IIR_LANE_BLOCK; ++i) iir_step(F, nsec, s, xl[i]);
#pragma unroll
  for (int c = 0; c < IIR_STATE; ++c) es[c * IIR_THREADS + lane] = s[c];
#pragma unroll
  for (int k = 0; k < IIR_SCAN_STEPS; ++k) {
    const int d = 1 << k;
    float v[IIR_STATE];
    __syncthreads();
    if (lane >= d) {
#pragma unroll
      for (int c = 0; c < IIR_STATE; ++c) v[c] = es[c * IIR_THREADS + lane - d];
    }
    __syncthreads();
    if (lane >= d) {
      const float* M = F.pw[k];
#pragma unroll
      for (int i = 0; i < IIR_STATE; ++i) {
        float acc = s[i];
#pragma unroll
        for (int j = 0; j < IIR_STATE; ++j) acc = acc + M[i * IIR_STATE + j] * v[j];
        s[i] = acc;
      }
#pragma unroll
      for (int c = 0; c < IIR_STATE; ++c) es[c * IIR_THREADS + lane] = s[c];
    }
  }
  if (!WRITE) {
    if (lane == IIR_THREADS - 1) {
#pragma unroll
      for (int c = 0; c < IIR_STATE; ++c) st[c] = s[c];
    }
    return;
  }
  __syncthreads();
  if (lane > 0) {
#pragma unroll
    for (int c = 0; c < IIR_STATE; ++c) s0[c] = es[c * IIR_THREADS + lane - 1];
  }
  for (int i = 0; i < IIR_LANE_BLOCK; ++i) xl[i] = iir_step(F, nsec, s0, xl[i]);
  __syncthreads();
  float* out = dst + (size_t)row * (mode == IIR_FORWARD ? ext : (size_t)n);
#pragma unroll 4
  for (int k = 0; k < IIR_LANE_BLOCK; ++k) {
    const int idx = k * IIR_THREADS + lane, p = t0 + idx;
    if (p >= m) break;
    const float y = xs[idx + (idx >> 5)];
    if (mode != IIR_BACKWARD) {
      out[p] = y;
    } else {
      const int q = m - 1 - p - pl;
      if (q >= 0 && q < n) out[q] = y;
    }
  }
}

constexpr int IIR_CARRY_CHUNK = 16;                        // tile states fetched ahead of the recurrence

__global__ __launch_bounds__(64) void iir_carry_kernel(const IirFilter* __restrict__ tab, int R,
                                                       const int32_t* __restrict__ row_filter, const float* src, float* states,
                                                       int n, int nt, int mode) {
  const int row = blockIdx.x, lane = threadIdx.x;
  const IirFilter& F = iir_filter(tab, R, row_filter, row);
  const int pl = F.padlen;
  const int m = mode == IIR_PLAIN ? n : n + 2 * pl;
  const int ntr = (m + IIR_TILE - 1) / IIR_TILE;
  const int i = lane < IIR_STATE ? lane : 0;               // the other lanes repeat coordinate 0 and store nothing
  float q[IIR_STATE];
#pragma unroll
  for (int j = 0; j < IIR_STATE; ++j) q[j] = F.pw[IIR_POWERS - 1][i * IIR_STATE + j];
  const float* in = src + (size_t)row * (mode == IIR_BACKWARD ? (size_t)n + 2 * IIR_MAX_PADLEN : (size_t)n);
  float s = mode == IIR_PLAIN ? 0.f : F.zi[i] * iir_load(in, mode, n, pl, m, 0);
  float* st = states + (size_t)row * nt * IIR_STATE;
  float e[IIR_CARRY_CHUNK], en[IIR_CARRY_CHUNK];
#pragma unroll
  for (int k = 0; k < IIR_CARRY_CHUNK; ++k) e[k] = k < ntr ? st[k * IIR_STATE + i] : 0.f;
  for (int t0 = 0; t0 < ntr; t0 += IIR_CARRY_CHUNK) {
#pragma unroll
    for (int k = 0; k < IIR_CARRY_CHUNK; ++k) {
      const int t = t0 + IIR_CARRY_CHUNK + k;
      en[k] = t < ntr ? st[(size_t)t * IIR_STATE + i] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < IIR_CARRY_CHUNK; ++k) {
      const int t = t0 + k;
      if (t < ntr) {                                       // the same in every lane
        if (lane < IIR_STATE) st[(size_t)t * IIR_STATE + i] = s;   // slot t: the state behind tile t becomes the state in front of it
        float acc = e[k];
#pragma unroll
        for (int j = 0; j < IIR_STATE; ++j) acc = acc + q[j] * __shfl(s, j, 64);
        s = acc;
      }
    }
#pragma unroll
    for (int k = 0; k < IIR_CARRY_CHUNK; ++k) e[k] = en[k];
  }
}

}  // namespace

hipError_t iir_pass_launch(const IirFilter* tab, int R, const int32_t* row_filter, const float* src, float* dst, float* states, int B,
                           int n, int mode, hipStream_t s) {
  const int nt = iir_tiles(n);
  const dim3 grid(nt, B);
  iir_tile_kernel<false><<<grid, IIR_THREADS, 0, s>>>(tab, R, row_filter, src, dst, states, n, nt, mode);
  iir_carry_kernel<<<B, 64, 0, s>>>(tab, R, row_filter, src, states, n, nt, mode);
  iir_tile_kernel<true><<<grid, IIR_THREADS, 0, s>>>(tab, R, row_filter, src, dst, states, n, nt, mode);
  return hipGetLastError();
}
