// Launchers of the harmonic kernels (harmonic.hip), used by jat_harmonic.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int HM_THREADS = 256;   // one block: 4 waves; analysis gives a wave one harmonic at a time
constexpr int HM_WAVE = 64;

// One configuration, every field already validated by jat_harmonic.cpp
struct HarmPlan {
  int N = 0, hop = 0, H = 0;      // frame_length, hop_length, n_harmonics
  double sr = 0.0, limit = 0.0;   // sample rate; analysis: sr / 2 - 2 sr / N, synthesis: sr / 2
};

// LDS of the analysis: the windowed frame [N] and the first half of the window [N / 2 + 1]
inline size_t harm_analyze_lds_bytes(const HarmPlan& p) { return ((size_t)p.N + (size_t)p.N / 2 + 4) * sizeof(float); }

// x [B, L], f0 / voiced [B, frames] -> amp [B, frames, H], energy [B, frames] (nullable).  A block walks the frames
// blockIdx.x, + gridDim.x, ..: a result does not depend on the grid.
hipError_t harm_analyze_launch(const HarmPlan& p, const float* x, int B, int64_t L, const float* f0, const uint8_t* voiced,
                               int frames, float* amp, float* energy, hipStream_t s);
// three launches: per-frame sums of the phase increments into work [B, frames], their exclusive scan per row in place, the samples
hipError_t harm_synth_launch(const HarmPlan& p, const float* f0, const uint8_t* voiced, const float* amp, int B, int frames,
                             int64_t L, float* y, uint32_t* phase, uint32_t* work, hipStream_t s);
// amp_a, amp_ref [B, frames, H], reference track [B, frames] -> out fp64 [B, 8], one block per row
hipError_t harm_compare_launch(const float* amp_a, const float* amp_ref, const float* f0_ref, const uint8_t* voiced_ref, int B,
                               int frames, int H, double cutoff_hz, double floor, double* out, hipStream_t s);
