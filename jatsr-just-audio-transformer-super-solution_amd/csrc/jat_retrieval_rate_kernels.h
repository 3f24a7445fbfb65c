// Launchers of the voicing-aware index-rate kernels (retrieval_rate.hip), used by jat_retrieval_rate.cpp.
#pragma once
#include "jat_retrieval_kernels.h"

constexpr int RR_MAX_HALF_WINDOW = 32;   // JAT_RATE_MAX_HALF_WINDOW
constexpr int RR_MAX_SMOOTH = 16;        // JAT_RATE_MAX_SMOOTH
constexpr int RR_MIX_ROWS = 4;           // channel rows one mix workgroup holds in flight per frame

// f0 fp32 [B, F], voiced uint8 [B, F] -> cls uint8 [B, F], count int32 [B, F] (may be null), summary int32 [B, 2] (may be
// null): one workgroup per row walks it in tiles of RT_THREADS frames with W frames of halo on either side.
hipError_t f0_classes_launch(const float* f0, const uint8_t* voiced, int B, int F, int W, float ratio, int min_count,
                             uint8_t* cls, int32_t* count, int32_t* summary, hipStream_t s);
// cls uint8 [B, F] -> r fp32 [B, T]: the table entry of every frame (frames t >= F: table[0]) smoothed over S frames on
// either side in the difference form.
hipError_t rate_track_launch(const uint8_t* cls, int B, int F, int T, float r0, float r1, float r2, int S, float* r,
                             hipStream_t s);
// y = fma(1 - r, x, r v) with r = rates[b, t]; x, v, y fp32 [B, C, T].
hipError_t rate_mix_launch(const float* x, const float* v, const float* rates, float* y, int B, int C, int T, hipStream_t s);
