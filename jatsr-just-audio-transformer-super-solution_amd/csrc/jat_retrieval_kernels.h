// Launchers of the latent-retrieval kernels (retrieval.hip), used by jat_retrieval.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int RT_THREADS = 256;      // every retrieval kernel: 4 waves
constexpr int RT_SLAB = 4096;        // key rows one search workgroup scans (JAT_BANK_SLAB)
constexpr int RT_QTILE = 32;         // queries per search workgroup, resident in LDS as two fp16 planes
constexpr int RT_KTILE = 128;        // key rows per step of the scan: one 32-row MFMA tile per wave
constexpr int RT_KCHUNK = 64;        // channels of the key tile staged in LDS at once
constexpr int RT_MIN_C = 32, RT_MAX_C = 1024;
constexpr int RT_MAX_K = 8;          // nearest rows per query at most (JAT_BANK_MAX_K)

struct RtPartial {   // one per (slab, query), or the list length of them for a top-k search
  float d;
  int32_t idx;
};

inline bool rt_channels_ok(int C) { return C >= RT_MIN_C && C <= RT_MAX_C && C % 32 == 0; }
// the list length a request for the k nearest rows runs with: the next of 1, 2, 4, 8
inline int rt_list_length(int k) { return k <= 1 ? 1 : k <= 2 ? 2 : k <= 4 ? 4 : 8; }

// rows[row0 + i, c] = fp16((float(src[c, first + i * stride]) - mean[c]) / std[c]) for i < count, and with src2 the same into
// rows2 with (mean2, std2).  src / src2: [C, len], fp16 or fp32.  The caller has checked first + (count - 1) * stride < len.
hipError_t bank_pack_launch(const void* src, const void* src2, bool src_fp16, int64_t len, int64_t first, int64_t stride,
                            int count, const float* mean, const float* std, const float* mean2, const float* std2,
                            uint16_t* rows, uint16_t* rows2, int64_t row0, int C, hipStream_t s);
// norms[row0 + i] = sum_c float(rows[row0 + i, c])^2 for i < count: one wave per row, a fixed order
hipError_t bank_norms_launch(const uint16_t* rows, float* norms, int64_t row0, int count, int C, hipStream_t s);
// x fp32 [B, C, T] -> idx int32 [B * T], dist2 fp32 [B * T] (may be null) over key rows [0, size); mean / std both null: x is
// used as it is.  part: ceil(size / RT_SLAB) * B * T entries.
hipError_t bank_search_launch(const uint16_t* keys, const float* norms, int size, int C, const float* x, const float* mean,
                              const float* std, int B, int T, int32_t* idx, float* dist2, RtPartial* part, hipStream_t s);
// The k nearest key rows of every query in ascending (d, index): idx int32 [B * T, k], dist2 fp32 [B * T, k] (may be null),
// unused places (size < k) idx -1 and dist2 +inf.  1 <= k <= RT_MAX_K; k = 1 is bank_search_launch.  part:
// ceil(size / RT_SLAB) * B * T * rt_list_length(k) entries.
hipError_t bank_search_topk_launch(const uint16_t* keys, const float* norms, int size, int C, const float* x,
                                   const float* mean, const float* std, int B, int T, int k, int32_t* idx, float* dist2,
                                   RtPartial* part, hipStream_t s);
// y = (1 - rate) x + rate v with v = sum_j w_j float(values[idx[b, t, j], c]) (* std[c] + mean[c] when given),
// w_j = u_j / sum_j u_j, u_j = (max(dist2_0, floor) / max(dist2_j, floor))^2 where idx_j >= 0 and 0 elsewhere; an index
// >= size is clamped, a negative one is not read
hipError_t bank_blend_topk_launch(const uint16_t* values, int size, int C, const float* x, const int32_t* idx,
                                  const float* dist2, int k, float floor, const float* mean, const float* std, float rate,
                                  float* y, int B, int T, hipStream_t s);
// y[b, c, t] = (1 - rate) x[b, c, t] + rate v,  v = float(values[idx[b, t], c]) (* std[c] + mean[c] when given); an index
// outside [0, size) is clamped into it
hipError_t bank_blend_launch(const uint16_t* values, int size, int C, const float* x, const int32_t* idx, const float* mean,
                             const float* std, float rate, float* y, int B, int T, hipStream_t s);

// ---- multi-scale retrieval (retrieval_ms.hip) -----------------------------------------------------------------
constexpr int RT_MAX_SCALES = 4;       // scales per multi-scale bank at most, each one of 1, 2, 4, 8
constexpr int RT_POOL_FRAMES = 256;    // frames of x one pooling workgroup reads: 32 windows of the widest scale

inline bool rt_scale_ok(int s) { return s == 1 || s == 2 || s == 4 || s == 8; }
struct RtPoolArgs {   // by value in the kernel's arguments: the scales > 1 of one launch and where each goes
  float* out[RT_MAX_SCALES - 1];       // [B, C, ceil(T / scale)]
  int scale[RT_MAX_SCALES - 1];
  int n;
};
struct RtMixArgs {    // by value: the tracks of one mix
  const float* v[RT_MAX_SCALES];       // [B, C, ceil(T / scale)]
  int scale[RT_MAX_SCALES];
  float a[RT_MAX_SCALES];              // the weights, normalised by the caller
  int n;
};
// bank_pack_launch with a window: row i pools the frames first + i * stride + j, j < min(window, len - frame), of each
// channel: normalised, summed in ascending order, divided by their number.  window = 1 writes what bank_pack_launch writes.
hipError_t bank_pack_pool_launch(const void* src, const void* src2, bool src_fp16, int64_t len, int64_t first, int64_t stride,
                                 int count, int window, const float* mean, const float* std, const float* mean2,
                                 const float* std2, uint16_t* rows, uint16_t* rows2, int64_t row0, int C, hipStream_t s);
// out_i[b, c, ts] = the pooled window of scale_i that starts at frame ts * scale_i of x[b, c, :] (normalised with mean / std
// when given), for every i < a.n in one launch; C a multiple of 32
hipError_t bank_pool_queries_launch(const float* x, const float* mean, const float* std, int B, int C, int T,
                                    const RtPoolArgs& a, hipStream_t s);
// y = (1 - rate) x + rate sum_i a_i u_i, u_i the track v_i interpolated linearly (half-pixel centres) to T frames; y may be x
hipError_t bank_mix_scales_launch(const float* x, const RtMixArgs& a, float rate, float* y, int B, int C, int T,
                                  hipStream_t s);
