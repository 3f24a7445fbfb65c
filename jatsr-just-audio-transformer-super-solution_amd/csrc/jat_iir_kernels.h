// Launchers of the IIR cascade kernels (iir.hip), used by jat_iir.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int IIR_SECTIONS = 5;                            // second-order sections of a padded cascade
constexpr int IIR_STATE = 2 * IIR_SECTIONS;                // state coordinates {s1, s2} per section
constexpr int IIR_LANE_BLOCK = 32;                         // consecutive samples a lane owns
constexpr int IIR_THREADS = 256;                           // lanes of a workgroup
constexpr int IIR_TILE = IIR_LANE_BLOCK * IIR_THREADS;     // samples of a workgroup
constexpr int IIR_SCAN_STEPS = 8;                          // log2(IIR_THREADS)
constexpr int IIR_POWERS = IIR_SCAN_STEPS + 1;             // P^(2^k), k = 0 .. 8; the last is A^IIR_TILE
constexpr int IIR_MAX_PADLEN = 3 * (2 * IIR_SECTIONS + 1);

// one filter of the device table, fp32
struct IirFilter {
  float c[IIR_SECTIONS][5];                                // b0 b1 b2 a1 a2
  float zi[IIR_STATE];
  int32_t nsec, padlen;
  int32_t pad[3];                                          // 16-byte multiples
  float pw[IIR_POWERS][IIR_STATE * IIR_STATE];             // row-major
};

enum IirMode { IIR_PLAIN = 0, IIR_FORWARD = 1, IIR_BACKWARD = 2 };

inline int iir_tiles(int64_t n) { return (int)((n + 2 * IIR_MAX_PADLEN + IIR_TILE - 1) / IIR_TILE); }

// One pass (A, B, C) over B rows.  IIR_PLAIN: src = x [B, n] -> dst = y [B, n], zero state.  IIR_FORWARD: src = x [B, n] -> dst =
// ext [B, n + 2 IIR_MAX_PADLEN], the filtered odd extension, from zi * its first sample.  IIR_BACKWARD: src = ext, read from its
// end, from zi * its last sample -> dst = y [B, n], the extension dropped.  states: [B, iir_tiles(n), IIR_STATE] floats.
hipError_t iir_pass_launch(const IirFilter* tab, int R, const int32_t* row_filter, const float* src, float* dst, float* states, int B,
                           int n, int mode, hipStream_t s);
