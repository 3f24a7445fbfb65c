// C ABI of latent retrieval (include/jat_hip.h): the bank handle, the argument checks and the launches of retrieval.hip.
// Every device buffer is allocated in jat_bank_create; add / search / blend only enqueue on the caller's stream.
#include "jat_internal.h"
#include "jat_retrieval_kernels.h"
#include "../../include/jat_hip_ms.h"

#include "jat_bank.h"   // struct jat_bank, shared with jat_retrieval_km.cpp

namespace {

constexpr int64_t kMax31 = 0x7fffffff;
static_assert(JAT_BANK_SLAB == RT_SLAB && JAT_BANK_MAX_K == RT_MAX_K && JAT_BANK_MAX_SCALES == RT_MAX_SCALES,
              "header and kernel disagree");

int check_bank(const char* who, const jat_bank* b) {
  if (!b) return fail(JAT_E_INVALID, "%s: null bank", who);
  return JAT_OK;
}

// B x T queries of `channels` channels: the element count of x and the grids fit
int check_queries(const char* who, const jat_bank* b, int32_t B, int32_t T) {
  if (B < 1 || B > 65535) return fail(JAT_E_INVALID, "%s: batch %d outside 1..65535", who, B);
  if (T < 1) return fail(JAT_E_INVALID, "%s: T %d must be at least 1", who, T);
  if ((int64_t)B * T > kMax31 / 2) return fail(JAT_E_INVALID, "%s: %d x %d queries do not fit 30 bits", who, B, T);
  return JAT_OK;
}

size_t search_bytes(const jat_bank* b, int64_t nq) {
  const size_t slabs = ((size_t)b->capacity + RT_SLAB - 1) / RT_SLAB;
  return align_up(slabs * (size_t)nq * sizeof(RtPartial), 256);
}

size_t topk_bytes(const jat_bank* b, int64_t nq, int k) {
  const size_t slabs = ((size_t)b->capacity + RT_SLAB - 1) / RT_SLAB;
  return align_up(slabs * (size_t)nq * rt_list_length(k) * sizeof(RtPartial), 256);
}

int check_k(const char* who, int32_t k) {
  if (k < 1 || k > JAT_BANK_MAX_K) return fail(JAT_E_INVALID, "%s: k %d outside 1..%d", who, k, JAT_BANK_MAX_K);
  return JAT_OK;
}

// what jat_bank_add and jat_bank_add_pooled refuse: `count` frames (window starts) first + i stride of a source of `len`
int check_add(const char* who, const jat_bank* bank, const void* key_src, const void* value_src, int64_t len, int64_t first,
              int64_t stride, int32_t count, const float* key_mean, const float* key_std, const float* value_mean,
              const float* value_std) {
  JCHK(check_bank(who, bank));
  if (!key_src || !key_mean || !key_std) return fail(JAT_E_INVALID, "%s: null key source or statistics", who);
  if (bank->paired ? (!value_src || !value_mean || !value_std) : (value_src != nullptr))
    return fail(JAT_E_INVALID, bank->paired ? "%s: a paired bank needs the value source and its statistics"
                                            : "%s: value source given to a bank that is not paired", who);
  if (len < 1 || len > kMax31 || first < 0 || stride < 1 || count < 1)
    return fail(JAT_E_INVALID, "%s: len %lld, first %lld, stride %lld, count %d", who, (long long)len, (long long)first,
                (long long)stride, count);
  if (first >= len || (int64_t)(count - 1) > (len - 1 - first) / stride)
    return fail(JAT_E_INVALID, "%s: frames %lld + %lld i, i < %d, leave the %lld frames of the source", who, (long long)first,
                (long long)stride, count, (long long)len);
  if ((int64_t)bank->size + count > bank->capacity)
    return fail(JAT_E_STATE, "%s: %d + %d rows exceed the capacity %d", who, bank->size, count, bank->capacity);
  return JAT_OK;
}

// [p, p + n floats) and [q, q + m floats) share a byte
bool overlap(const float* p, int64_t n, const float* q, int64_t m) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + (uintptr_t)m * sizeof(float) && b < a + (uintptr_t)n * sizeof(float);
}

// n scales, strictly ascending, each one of 1, 2, 4, 8 and at least `least`
int check_scale_list(const char* who, int32_t n, const int32_t* scales, int most, int least) {
  if (n < 1 || n > most) return fail(JAT_E_INVALID, "%s: %d scales outside 1..%d", who, n, most);
  if (!scales) return fail(JAT_E_INVALID, "%s: null scales", who);
  for (int i = 0; i < n; ++i) {
    if (!rt_scale_ok(scales[i]) || scales[i] < least)
      return fail(JAT_E_INVALID, "%s: scale %d is not one of%s 2, 4, 8", who, scales[i], least > 1 ? "" : " 1,");
    if (i && scales[i] <= scales[i - 1])
      return fail(JAT_E_INVALID, "%s: scales must ascend strictly (%d after %d)", who, scales[i], scales[i - 1]);
  }
  return JAT_OK;
}

void release(jat_bank* b) {
  if (b->paired && b->values) (void)hipFree(b->values);
  if (b->keys) (void)hipFree(b->keys);
  if (b->norms) (void)hipFree(b->norms);
  delete b;
}

}  // namespace

extern "C" {

int jat_bank_create(int32_t channels, int32_t capacity, int32_t paired, jat_bank** out) {
  if (!out) return fail(JAT_E_INVALID, "jat_bank_create: null output pointer");
  *out = nullptr;
  if (!rt_channels_ok(channels))
    return fail(JAT_E_INVALID, "jat_bank_create: channels %d must be a multiple of 32 in %d..%d", channels, RT_MIN_C, RT_MAX_C);
  if (capacity < 1 || (int64_t)capacity > (int64_t)65535 * RT_SLAB)
    return fail(JAT_E_INVALID, "jat_bank_create: capacity %d outside 1..%lld", capacity, (long long)65535 * RT_SLAB);
  jat_bank* b = new jat_bank;
  b->channels = channels, b->capacity = capacity, b->paired = paired != 0;
  const size_t row_bytes = (size_t)capacity * channels * sizeof(uint16_t);
  const size_t norm_bytes = align_up((size_t)capacity, RT_KTILE) * sizeof(float);
  hipError_t e = hipMalloc((void**)&b->keys, row_bytes);
  if (e == hipSuccess) e = hipMalloc((void**)&b->norms, norm_bytes);
  if (e == hipSuccess && b->paired) e = hipMalloc((void**)&b->values, row_bytes);
  if (e == hipSuccess) e = hipMemset(b->norms, 0, norm_bytes);
  if (e != hipSuccess) {
    release(b);
    return fail(JAT_E_HIP, "jat_bank_create: %d rows of %d channels: %s", capacity, channels, hipGetErrorString(e));
  }
  if (!b->paired) b->values = b->keys;
  *out = b;
  return JAT_OK;
}

void jat_bank_destroy(jat_bank* bank) {
  if (bank) release(bank);
}

int jat_bank_size(const jat_bank* bank, int32_t* size) {
  JCHK(check_bank("jat_bank_size", bank));
  if (!size) return fail(JAT_E_INVALID, "jat_bank_size: null output pointer");
  *size = bank->size;
  return JAT_OK;
}

int jat_bank_clear(jat_bank* bank) {
  JCHK(check_bank("jat_bank_clear", bank));
  bank->size = 0;
  return JAT_OK;
}

int jat_bank_add(jat_bank* bank, const void* key_src, const void* value_src, int32_t src_is_fp16, int64_t len, int64_t first,
                 int64_t stride, int32_t count, const float* key_mean, const float* key_std, const float* value_mean,
                 const float* value_std, void* stream) {
  JCHK(check_add("jat_bank_add", bank, key_src, value_src, len, first, stride, count, key_mean, key_std, value_mean, value_std));
  hipStream_t s = (hipStream_t)stream;
  KCHK(bank_pack_launch(key_src, bank->paired ? value_src : nullptr, src_is_fp16 != 0, len, first, stride, count, key_mean,
                        key_std, value_mean, value_std, bank->keys, bank->values, bank->size, bank->channels, s));
  KCHK(bank_norms_launch(bank->keys, bank->norms, bank->size, count, bank->channels, s));
  bank->size += count;
  return JAT_OK;
}

int jat_bank_rows(const jat_bank* bank, int32_t which, const void** rows, const float** norms) {
  JCHK(check_bank("jat_bank_rows", bank));
  if (which != JAT_BANK_KEYS && which != JAT_BANK_VALUES) return fail(JAT_E_INVALID, "jat_bank_rows: which %d", which);
  if (!rows) return fail(JAT_E_INVALID, "jat_bank_rows: null output pointer");
  *rows = which == JAT_BANK_KEYS ? bank->keys : bank->values;
  if (norms) *norms = (which == JAT_BANK_KEYS || !bank->paired) ? bank->norms : nullptr;
  return JAT_OK;
}

int jat_bank_load_rows(jat_bank* bank, const void* keys, const void* values, int32_t count, void* stream) {
  JCHK(check_bank("jat_bank_load_rows", bank));
  if (!keys || (bank->paired ? !values : values != nullptr))
    return fail(JAT_E_INVALID, "jat_bank_load_rows: keys, and values exactly when the bank is paired");
  if (count < 1) return fail(JAT_E_INVALID, "jat_bank_load_rows: count %d must be at least 1", count);
  if ((int64_t)bank->size + count > bank->capacity)
    return fail(JAT_E_STATE, "jat_bank_load_rows: %d + %d rows exceed the capacity %d", bank->size, count, bank->capacity);
  hipStream_t s = (hipStream_t)stream;
  const size_t off = (size_t)bank->size * bank->channels, bytes = (size_t)count * bank->channels * sizeof(uint16_t);
  HIPCHK(hipMemcpyAsync(bank->keys + off, keys, bytes, hipMemcpyDeviceToDevice, s));
  if (bank->paired) HIPCHK(hipMemcpyAsync(bank->values + off, values, bytes, hipMemcpyDeviceToDevice, s));
  KCHK(bank_norms_launch(bank->keys, bank->norms, bank->size, count, bank->channels, s));
  bank->size += count;
  return JAT_OK;
}

int jat_bank_search_workspace_bytes(const jat_bank* bank, int64_t n_queries, size_t* bytes) {
  JCHK(check_bank("jat_bank_search_workspace_bytes", bank));
  if (!bytes) return fail(JAT_E_INVALID, "jat_bank_search_workspace_bytes: null output pointer");
  if (n_queries < 1 || n_queries > kMax31 / 2)
    return fail(JAT_E_INVALID, "jat_bank_search_workspace_bytes: %lld queries outside 1..2^30", (long long)n_queries);
  *bytes = search_bytes(bank, n_queries);
  return JAT_OK;
}

int jat_bank_search(jat_bank* bank, const float* x, const float* mean, const float* std, int32_t B, int32_t T, int32_t* idx,
                    float* dist2, void* work, size_t work_bytes, void* stream) {
  JCHK(check_bank("jat_bank_search", bank));
  JCHK(check_queries("jat_bank_search", bank, B, T));
  if (!x || !idx || !work) return fail(JAT_E_INVALID, "jat_bank_search: null buffer");
  if ((mean != nullptr) != (std != nullptr)) return fail(JAT_E_INVALID, "jat_bank_search: mean and std are both given or both null");
  if ((uintptr_t)work & 7) return fail(JAT_E_INVALID, "jat_bank_search: the workspace must be 8-byte aligned");
  const size_t need = search_bytes(bank, (int64_t)B * T);
  if (work_bytes < need) return fail(JAT_E_INVALID, "jat_bank_search: workspace %zu < %zu bytes", work_bytes, need);
  if (bank->size < 1) return fail(JAT_E_STATE, "jat_bank_search: the bank is empty");
  KCHK(bank_search_launch(bank->keys, bank->norms, bank->size, bank->channels, x, mean, std, B, T, idx, dist2, (RtPartial*)work,
                          (hipStream_t)stream));
  return JAT_OK;
}

int jat_bank_blend(jat_bank* bank, const float* x, const int32_t* idx, const float* value_mean, const float* value_std,
                   float rate, float* y, int32_t B, int32_t T, void* stream) {
  JCHK(check_bank("jat_bank_blend", bank));
  JCHK(check_queries("jat_bank_blend", bank, B, T));
  if (!x || !idx || !y) return fail(JAT_E_INVALID, "jat_bank_blend: null buffer");
  if ((value_mean != nullptr) != (value_std != nullptr))
    return fail(JAT_E_INVALID, "jat_bank_blend: value_mean and value_std are both given or both null");
  if (!(rate >= 0.f && rate <= 1.f)) return fail(JAT_E_INVALID, "jat_bank_blend: index rate %g outside [0, 1]", (double)rate);
  if (bank->size < 1) return fail(JAT_E_STATE, "jat_bank_blend: the bank is empty");
  KCHK(bank_blend_launch(bank->values, bank->size, bank->channels, x, idx, value_mean, value_std, rate, y, B, T,
                         (hipStream_t)stream));
  return JAT_OK;
}

int jat_bank_topk_workspace_bytes(const jat_bank* bank, int64_t n_queries, int32_t k, size_t* bytes) {
  JCHK(check_bank("jat_bank_topk_workspace_bytes", bank));
  if (!bytes) return fail(JAT_E_INVALID, "jat_bank_topk_workspace_bytes: null output pointer");
  if (n_queries < 1 || n_queries > kMax31 / 2)
    return fail(JAT_E_INVALID, "jat_bank_topk_workspace_bytes: %lld queries outside 1..2^30", (long long)n_queries);
  JCHK(check_k("jat_bank_topk_workspace_bytes", k));
  *bytes = topk_bytes(bank, n_queries, k);
  return JAT_OK;
}

int jat_bank_search_topk(jat_bank* bank, const float* x, const float* mean, const float* std, int32_t B, int32_t T, int32_t k,
                         int32_t* idx, float* dist2, void* work, size_t work_bytes, void* stream) {
  JCHK(check_bank("jat_bank_search_topk", bank));
  JCHK(check_queries("jat_bank_search_topk", bank, B, T));
  JCHK(check_k("jat_bank_search_topk", k));
  if (!x || !idx || !work) return fail(JAT_E_INVALID, "jat_bank_search_topk: null buffer");
  if ((mean != nullptr) != (std != nullptr))
    return fail(JAT_E_INVALID, "jat_bank_search_topk: mean and std are both given or both null");
  if ((uintptr_t)work & 7) return fail(JAT_E_INVALID, "jat_bank_search_topk: the workspace must be 8-byte aligned");
  const size_t need = topk_bytes(bank, (int64_t)B * T, k);
  if (work_bytes < need) return fail(JAT_E_INVALID, "jat_bank_search_topk: workspace %zu < %zu bytes", work_bytes, need);
  if (bank->size < 1) return fail(JAT_E_STATE, "jat_bank_search_topk: the bank is empty");
  KCHK(bank_search_topk_launch(bank->keys, bank->norms, bank->size, bank->channels, x, mean, std, B, T, k, idx, dist2,
                               (RtPartial*)work, (hipStream_t)stream));
  return JAT_OK;
}

int jat_bank_blend_topk(jat_bank* bank, const float* x, const int32_t* idx, const float* dist2, int32_t k,
                        const float* value_mean, const float* value_std, float rate, float dist2_floor, float* y, int32_t B,
                        int32_t T, void* stream) {
  JCHK(check_bank("jat_bank_blend_topk", bank));
  JCHK(check_queries("jat_bank_blend_topk", bank, B, T));
  JCHK(check_k("jat_bank_blend_topk", k));
  if (!x || !idx || !dist2 || !y) return fail(JAT_E_INVALID, "jat_bank_blend_topk: null buffer");
  if ((value_mean != nullptr) != (value_std != nullptr))
    return fail(JAT_E_INVALID, "jat_bank_blend_topk: value_mean and value_std are both given or both null");
  if (!(rate >= 0.f && rate <= 1.f))
    return fail(JAT_E_INVALID, "jat_bank_blend_topk: index rate %g outside [0, 1]", (double)rate);
  if (!(dist2_floor > 0.f) || dist2_floor == __builtin_inff())
    return fail(JAT_E_INVALID, "jat_bank_blend_topk: dist2_floor %g must be positive and finite", (double)dist2_floor);
  if (bank->size < 1) return fail(JAT_E_STATE, "jat_bank_blend_topk: the bank is empty");
  KCHK(bank_blend_topk_launch(bank->values, bank->size, bank->channels, x, idx, dist2, k, dist2_floor, value_mean, value_std,
                              rate, y, B, T, (hipStream_t)stream));
  return JAT_OK;
}

// ---- multi-scale retrieval (include/jat_hip_ms.h) ----------------------------------------------------------------------------
int jat_bank_add_pooled(jat_bank* bank, const void* key_src, const void* value_src, int32_t src_is_fp16, int64_t len,
                        int64_t first, int64_t stride, int32_t count, int32_t window, const float* key_mean,
                        const float* key_std, const float* value_mean, const float* value_std, void* stream) {
  JCHK(check_add("jat_bank_add_pooled", bank, key_src, value_src, len, first, stride, count, key_mean, key_std, value_mean,
                 value_std));
  if (!rt_scale_ok(window)) return fail(JAT_E_INVALID, "jat_bank_add_pooled: window %d is not one of 1, 2, 4, 8", window);
  hipStream_t s = (hipStream_t)stream;
  KCHK(bank_pack_pool_launch(key_src, bank->paired ? value_src : nullptr, src_is_fp16 != 0, len, first, stride, count, window,
                             key_mean, key_std, value_mean, value_std, bank->keys, bank->values, bank->size, bank->channels,
                             s));
  KCHK(bank_norms_launch(bank->keys, bank->norms, bank->size, count, bank->channels, s));
  bank->size += count;
  return JAT_OK;
}

int jat_bank_pool_frames(const float* x, const float* mean, const float* std, int32_t B, int32_t C, int32_t T, int32_t n,
                         const int32_t* scales, float* const* outs, void* stream) {
  JCHK(check_queries("jat_bank_pool_frames", nullptr, B, T));
  if (!rt_channels_ok(C))
    return fail(JAT_E_INVALID, "jat_bank_pool_frames: channels %d must be a multiple of 32 in %d..%d", C, RT_MIN_C, RT_MAX_C);
  if (!x || !outs) return fail(JAT_E_INVALID, "jat_bank_pool_frames: null buffer");
  if ((mean != nullptr) != (std != nullptr))
    return fail(JAT_E_INVALID, "jat_bank_pool_frames: mean and std are both given or both null");
  JCHK(check_scale_list("jat_bank_pool_frames", n, scales, RT_MAX_SCALES - 1, 2));
  RtPoolArgs a = {};
  a.n = n;
  for (int i = 0; i < n; ++i) {
    const int64_t Ts = ((int64_t)T + scales[i] - 1) / scales[i];
    if (!outs[i]) return fail(JAT_E_INVALID, "jat_bank_pool_frames: null output for scale %d", scales[i]);
    if (overlap(x, (int64_t)B * C * T, outs[i], (int64_t)B * C * Ts))
      return fail(JAT_E_INVALID, "jat_bank_pool_frames: the output of scale %d overlaps x", scales[i]);
    a.out[i] = outs[i], a.scale[i] = scales[i];
  }
  KCHK(bank_pool_queries_launch(x, mean, std, B, C, T, a, (hipStream_t)stream));
  return JAT_OK;
}

int jat_bank_mix_scales(const float* x, int32_t n, const int32_t* scales, const float* const* tracks, const float* weights,
                        float rate, float* y, int32_t B, int32_t C, int32_t T, void* stream) {
  JCHK(check_queries("jat_bank_mix_scales", nullptr, B, T));
  if (C < 1 || C > RT_MAX_C) return fail(JAT_E_INVALID, "jat_bank_mix_scales: channels %d outside 1..%d", C, RT_MAX_C);
  if (!x || !y || !tracks || !weights) return fail(JAT_E_INVALID, "jat_bank_mix_scales: null buffer");
  if (!(rate >= 0.f && rate <= 1.f))
    return fail(JAT_E_INVALID, "jat_bank_mix_scales: index rate %g outside [0, 1]", (double)rate);
  JCHK(check_scale_list("jat_bank_mix_scales", n, scales, RT_MAX_SCALES, 1));
  RtMixArgs a = {};
  a.n = n;
  for (int i = 0; i < n; ++i) {
    const int64_t Ts = ((int64_t)T + scales[i] - 1) / scales[i];
    if (!tracks[i]) return fail(JAT_E_INVALID, "jat_bank_mix_scales: null track for scale %d", scales[i]);
    if (!(weights[i] > 0.f) || weights[i] == __builtin_inff())
      return fail(JAT_E_INVALID, "jat_bank_mix_scales: weight %g of scale %d must be positive and finite", (double)weights[i],
                  scales[i]);
    if (overlap(y, (int64_t)B * C * T, tracks[i], (int64_t)B * C * Ts))
      return fail(JAT_E_INVALID, "jat_bank_mix_scales: the track of scale %d overlaps y", scales[i]);
    a.v[i] = tracks[i], a.scale[i] = scales[i], a.a[i] = weights[i];
  }
  KCHK(bank_mix_scales_launch(x, a, rate, y, B, C, T, (hipStream_t)stream));
  return JAT_OK;
}

}  // extern "C"
