// Launchers of the IVF index kernels (retrieval_ivf.hip), used by jat_retrieval_ivf.cpp.
#pragma once
#include "jat_retrieval_kernels.h"

constexpr int IVF_MAX_NPROBE = 8;        // JAT_IVF_MAX_NPROBE
constexpr int IVF_MAX_ROWS = 1 << 22;    // JAT_IVF_MAX_ROWS: the assignment's limit
constexpr int IVF_TILE = 32;             // list rows per MFMA tile: one wave's A operand

inline int ivf_padded_channels(int C) { return (C + RT_KCHUNK - 1) / RT_KCHUNK * RT_KCHUNK; }

// Groups the N rows of a bank by list: offsets int32 [nlist + 1], order int32 [N] (ascending source rows inside a list, rows
// whose idx is outside [0, nlist) behind all lists), and dst row p = src row order[p] (keys, values when given, norms).
// cursor: int32 [nlist + 1]; members: int32 [N].
hipError_t ivf_group_launch(const uint16_t* skeys, const uint16_t* svals, const float* snorms, const int32_t* idx, int N,
                            int nlist, int C, uint16_t* dkeys, uint16_t* dvals, float* dnorms, int32_t* offsets,
                            int32_t* order, int32_t* cursor, int32_t* members, hipStream_t s);
// x fp32 [B, C, T] -> the query planes qhi, qlo fp16 [B T, Cp] (Cp = ivf_padded_channels(C), channels >= C zeros) and
// qn fp32 [B T] = |q|^2, all three as bank_search_kernel computes them
hipError_t ivf_prepare_launch(const float* x, const float* mean, const float* std, int B, int T, int C, uint16_t* qhi,
                              uint16_t* qlo, float* qn, hipStream_t s);
// The first k rows by (d, position) among the lists probes[n, 0 .. nprobe) of query n (an entry outside [0, nlist) probes
// nothing): idx int32 [nq, k], dist2 fp32 [nq, k] (may be null), unused places idx -1 and dist2 +inf.
hipError_t ivf_scan_launch(const uint16_t* keys, const float* norms, int size, int C, const int32_t* offsets, int nlist,
                           const int32_t* probes, int nprobe, const uint16_t* qhi, const uint16_t* qlo, const float* qn,
                           int64_t nq, int k, int32_t* idx, float* dist2, hipStream_t s);
