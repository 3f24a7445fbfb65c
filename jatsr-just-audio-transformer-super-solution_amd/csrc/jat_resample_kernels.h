// Launchers of the sample-rate converter and the per-channel statistics kernels (resample.hip), used by jat_resample.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int RS_FRAMES = 8;           // output frames a thread accumulates in registers
constexpr int RS_TAP_TILE = 8;         // taps whose table entries are loaded ahead of their use
constexpr int RS_MAX_THREADS = 256;
constexpr int RS_MAX_WINDOW = 12288;   // floats of staged input per block (48 KiB of LDS)
constexpr int STATS_SLICES = 16;       // partial sums per channel (= JAT_STATS_SLICES)

// How one block is cut: each thread owns `ph` phases (l, l + lanes, ...) of `frames` = groups * RS_FRAMES frames.
struct ResampleGeom {
  int ph = 1;       // phases per thread: 1 or 4
  int pn = 0;       // phases per block (one phase slice)
  int lanes = 0;    // threads per frame group = ceil(pn / ph)
  int groups = 0;   // most frame groups per block (a launch may take fewer); blockDim = lanes * groups
  int slices = 0;   // gridDim.y = ceil(n / pn)
};
// false when no block shape keeps the staged window within RS_MAX_WINDOW
bool resample_geometry(int o, int n, int K, ResampleGeom* g);

// One launch over rows of L_out outputs: the frame groups pick_groups gives its n_frames = ceil(L_out / n) frames, and the
// grid, block and dynamic LDS that follow.  resample_launch launches by it; jat_k_resample_geometry reports it.
struct ResampleLaunch {
  int groups = 0;      // frame groups per block of this launch (<= ResampleGeom::groups)
  int fpb = 0;         // frames per block = groups * RS_FRAMES
  int n_frames = 0;
  unsigned grid_x = 0; // blocks along the frames; gridDim = (grid_x, slices, B)
  int block = 0;       // threads = lanes * groups
  size_t lds = 0;      // bytes of the staged window: ((fpb - 1) o + K) floats
};
ResampleLaunch resample_launch_shape(const ResampleGeom& g, int L_out, int o, int n, int K);

// y[b, f n + p] = sum_k ht[k, p] * x[b, f o + k - width] (x = 0 outside [0, L)); ht is the tap table transposed to [K, n]
hipError_t resample_launch(const float* x, float* y, const float* ht, int B, int L, int L_out, int o, int n, int width, int K,
                           const ResampleGeom& g, hipStream_t s);
// sum[c] += sum_{b,t} h(z[b, c, t]), sq[c] += sum h(z)^2 with h = rounding to fp16, in fp64; partial: [C, STATS_SLICES, 2] doubles
hipError_t channel_stats_launch(const float* z, int B, int C, int T, double* partial, double* sum, double* sq, hipStream_t s);
