// Launchers of the k-means compaction kernels (retrieval_km.hip), used by jat_retrieval_km.cpp.
#pragma once
#include "jat_retrieval_kernels.h"

constexpr int KM_QTILE = 64;              // pool rows per assignment workgroup, resident in LDS as one fp16 plane
constexpr int KM_CTILE = 128;             // channels per segmented-sum workgroup: 64 lanes x 2 halves
constexpr int KM_MAX_POOL = 1 << 22;      // JAT_KM_MAX_POOL

// idx[n], dist2[n] (may be null) for pool rows first + n, n < count, over centroid rows [0, K); *changed (may be null) +=
// the number of n whose idx[n] differed on entry.  cnorms has whole RT_KTILE groups allocated (jat_bank_create).
hipError_t km_assign_launch(const uint16_t* pool, const float* pnorms, int64_t first, int count, const uint16_t* cent,
                            const float* cnorms, int K, int C, int32_t* idx, float* dist2, int32_t* changed, hipStream_t s);
// counts[i] = members of cluster i; every cluster with members gets the mean of its members' rows (keys, and values when
// pvals / cvals are given) as defined in include/jat_hip_km.h.  offsets, cursor: int32 [K]; members: int32 [N].  An idx entry
// outside [0, K) is skipped.
hipError_t km_update_launch(const uint16_t* pkeys, const uint16_t* pvals, const int32_t* idx, int N, uint16_t* ckeys,
                            uint16_t* cvals, int K, int C, int32_t* counts, int32_t* offsets, int32_t* cursor,
                            int32_t* members, hipStream_t s);
// out[0] = sum of d[0 .. n) in fp64, a fixed order
hipError_t km_sum_dist2_launch(const float* d, int64_t n, double* out, hipStream_t s);
