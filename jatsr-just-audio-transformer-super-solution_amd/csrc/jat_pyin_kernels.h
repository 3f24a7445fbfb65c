// Launchers of the pYIN kernels (pyin.hip), used by jat_pyin.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int PY_THREADS = 256;        // pyin_observe_kernel: one block, one frame at a time
constexpr int PY_CHUNK = 16;           // troughs whose threshold terms are transposed through LDS at a time
constexpr int PY_TILE_STRIDE = 264;    // floats per trough in that tile: >= PY_MAX_THRESHOLDS, 8 mod 32
constexpr int PY_MAX_THRESHOLDS = 256; // one thread of the observe block per threshold
constexpr int PY_MAX_BINS = 1024;      // one thread of the Viterbi block per pitch bin
constexpr int PY_MAX_H = 128;          // widest transition: 2 H + 1 = 257 sources per target
constexpr int PY_MAX_NY = 4096;        // candidates per frame (frame_length 8192 gives at most 4095 lags)

// One pYIN configuration, every field validated by jat_pyin.cpp; the pointers are device tables owned by the handle
struct PyinPlan {
  int min_period = 0, ny = 0, lags = 0;     // y[i] = cmndf[min_period + i], i < ny; lags = max_period + 1 floats per cmndf row
  int n_thresholds = 0, n_bins = 0, H = 0, nt_max = 0;
  double sr = 0.0, fmin = 0.0, bin_scale = 0.0;   // bin position = bin_scale * log2(f0 / fmin), bin_scale = 12 bps
  float no_trough_prob = 0.f, lk = 0.f, ls = 0.f, logpi = 0.f;
  const float* theta = nullptr;      // [N + 2]: theta[m] = fp32(m / N), m = 1 .. N; theta[0] = -inf, theta[N + 1] = +inf
  const float* beta = nullptr;       // [N + 1]: beta[m], m = 1 .. N
  const float* cum_beta = nullptr;   // [N + 2]: cum_beta[q] = sum_{m < q} beta_m, q = 1 .. N + 1
  const float* A = nullptr;          // [nt_max + 1]: (1 - e^-lambda) e^(-lambda p)
  const float* invD = nullptr;       // [nt_max + 1]: 1 / (1 - e^(-lambda n)), n >= 1
  const float* logw = nullptr;       // [2 H + 1]
  const float* logZ = nullptr;       // [n_bins]
  const float* freqs = nullptr;      // [n_bins]
};

inline size_t pyin_observe_lds_bytes(const PyinPlan& p) {
  // y[ny] | prob[nt_max] | tile[PY_CHUNK][PY_TILE_STRIDE] | win[n_bins] (int) | tk, tq, tb [nt_max] (uint16, an even count each)
  return ((size_t)p.ny + p.nt_max + PY_CHUNK * PY_TILE_STRIDE + p.n_bins) * 4 + ((size_t)p.nt_max + 1) / 2 * 2 * 2 * 3;
}
// frames of back-pointers staged at a time by the back-trace: what fits 48 KiB, at least 12 (n_bins <= 1024), at most 192
constexpr int PY_TRACE_MAX = 192;
__host__ __device__ inline int pyin_trace_frames(const PyinPlan& p) {
  const int n = (int)(49152 / ((size_t)4 * p.n_bins));
  return n < PY_TRACE_MAX ? n : PY_TRACE_MAX;
}
inline size_t pyin_viterbi_lds_bytes(const PyinPlan& p) {     // U [n_bins + 2 H] float2, the reversed logw [2 H + 1]
  return ((size_t)p.n_bins + 2 * p.H) * 8 + ((size_t)2 * p.H + 1) * 4;
}
inline size_t pyin_trace_lds_bytes(const PyinPlan& p) { return (size_t)pyin_trace_frames(p) * 4 * p.n_bins; }

// cmndf fp32 [B, frames, lags] -> voiced_prob fp32 [B, frames], log_obs fp32 [B, frames, n_bins + 1]; nullable: prob fp32 and
// bin int32 [B, frames, ny], obs fp32 [B, frames, n_bins].  A block walks frames blockIdx.x, + gridDim.x, ...
hipError_t pyin_observe_launch(const PyinPlan& p, const float* cmndf, int B, int frames, float* voiced_prob, float* log_obs,
                               float* prob, int32_t* bin, float* obs, hipStream_t s);
// log_obs -> back: uint16 [B, frames, 2 n_bins] back-pointers, and the last state into state[b, frames - 1].  One block per row.
hipError_t pyin_forward_launch(const PyinPlan& p, const float* log_obs, int B, int frames, uint16_t* back, int32_t* state,
                               hipStream_t s);
// back and state[b, frames - 1] -> state int32, f0 fp32 and voiced uint8 [B, frames].  One block per row.
hipError_t pyin_trace_launch(const PyinPlan& p, int B, int frames, const uint16_t* back, int32_t* state, float* f0,
                             uint8_t* voiced, hipStream_t s);
