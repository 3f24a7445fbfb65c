// Launchers of the training-data kernels (data.hip), used by jat_data.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int DT_THREADS = 256;        // one gather block: 4 waves, one output row each
constexpr int DT_ROWS = DT_THREADS / 64;
constexpr int DT_MAX_FRAMES = 8176;    // four LDS rows of T + 14 halves in whole 16-byte chunks fill 64 KiB
constexpr int MON_THREADS = 256;
constexpr int MON_BLOCKS = 1024;       // first-stage blocks of the monitor: a constant, so the sum order never depends on the device
constexpr int MON_SUMS = 6;

// One launch for both tensors: rows [0, B*C) are hr_out's, rows [B*C, 2*B*C) lr_out's.  Tables are device arrays of B
// entries; the four statistics vectors are all given or all null.
hipError_t latent_gather_launch(const void* const* hr_src, const void* const* lr_src, const int64_t* len, const int64_t* start,
                                const float* hr_mean, const float* hr_std, const float* lr_mean, const float* lr_std,
                                float* hr_out, float* lr_out, int B, int C, int T, hipStream_t s);
// partial: MON_BLOCKS * MON_SUMS doubles; out: MON_SUMS doubles.  cond may be null (its two sums are then 0).
hipError_t train_monitor_launch(const float* pred, const float* target, const float* cond, int64_t n, double* partial,
                                double* out, hipStream_t s);
