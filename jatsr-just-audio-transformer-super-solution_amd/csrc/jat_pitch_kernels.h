// Launchers of the pitch kernels (pitch.hip), used by jat_pitch.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int PT_THREADS = 256;   // one block: 4 waves, one frame at a time
constexpr int PT_LAGS = 4;        // consecutive lags a thread owns (one aligned 16-byte LDS slot of x[j + tau])
constexpr int PT_PAD = 8;         // zero floats behind the staged frame: the sliding window of the last lag quad reads them

// One YIN configuration, every field already validated by jat_pitch.cpp
struct YinPlan {
  int frame_length = 0, hop = 0, W = 0;     // W = frame_length / 2 terms per lag
  int min_period = 0, max_period = 0;       // candidates y[i] = cmndf[min_period + i], i = 0 .. max_period - min_period
  float sr = 0.f, threshold = 0.f;
};

inline size_t yin_lds_bytes(const YinPlan& p) {
  const size_t frame = ((size_t)p.frame_length + 3) / 4 * 4 + PT_PAD, lags = ((size_t)p.max_period + 1 + 3) / 4 * 4;
  return (frame + lags) * sizeof(float);
}

// x fp32 [B, L] -> f0, aperiodicity fp32 [B, frames], voiced uint8 [B, frames]; nullable: index int32 [B, frames],
// d and cmndf fp32 [B, frames, max_period + 1].  A block walks frames b * frames + f = blockIdx.x, + gridDim.x, ...: a
// result does not depend on the grid.
hipError_t yin_launch(const YinPlan& p, const float* x, int B, int64_t L, int frames, float* f0, float* aperiodicity,
                      uint8_t* voiced, int32_t* index, float* d, float* cmndf, hipStream_t s);
// two tracks (f0 fp32, voiced uint8) [B, frames] -> out fp64 [B, 6], one block per row
hipError_t f0_compare_launch(const float* f0_a, const uint8_t* voiced_a, const float* f0_b, const uint8_t* voiced_b, int B,
                             int frames, double gross_cents, double* out, hipStream_t s);
