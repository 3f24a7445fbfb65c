// C ABI of the voicing-aware index rates (include/jat_hip_rate.h): the argument checks and the launches of
// retrieval_rate.hip.  Stateless; nothing here allocates, synchronises or copies.
#include <cmath>

#include "jat_internal.h"
#include "jat_retrieval_rate_kernels.h"
#include "../../include/jat_hip_rate.h"

namespace {

static_assert(JAT_RATE_MAX_HALF_WINDOW == RR_MAX_HALF_WINDOW && JAT_RATE_MAX_SMOOTH == RR_MAX_SMOOTH,
              "header and kernel disagree");

int check_batch(const char* who, int32_t B) {
  if (B < 1 || B > 65535) return fail(JAT_E_INVALID, "%s: batch %d outside 1..65535", who, B);
  return JAT_OK;
}

// [p, p + n bytes) and [q, q + m bytes) share a byte
bool overlap(const void* p, uint64_t n, const void* q, uint64_t m) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + m && b < a + n;
}

}  // namespace

extern "C" {

int jat_f0_classes(const float* f0, const uint8_t* voiced, int32_t B, int32_t F, int32_t half_window, float ratio,
                   int32_t min_count, uint8_t* cls, int32_t* count, int32_t* summary, void* stream) {
  JCHK(check_batch("jat_f0_classes", B));
  if (F < 1) return fail(JAT_E_INVALID, "jat_f0_classes: %d frames, must be at least 1", F);
  if (half_window < 0 || half_window > JAT_RATE_MAX_HALF_WINDOW)
    return fail(JAT_E_INVALID, "jat_f0_classes: half_window %d outside 0..%d", half_window, JAT_RATE_MAX_HALF_WINDOW);
  if (!(ratio > 1.f) || !std::isfinite(ratio))
    return fail(JAT_E_INVALID, "jat_f0_classes: ratio %g must be finite and above 1", (double)ratio);
  if (min_count < 1 || min_count > 2 * half_window + 1)
    return fail(JAT_E_INVALID, "jat_f0_classes: min_count %d outside 1..%d", min_count, 2 * half_window + 1);
  if (!f0 || !voiced || !cls) return fail(JAT_E_INVALID, "jat_f0_classes: null buffer");
  KCHK(f0_classes_launch(f0, voiced, B, F, half_window, ratio, min_count, cls, count, summary, (hipStream_t)stream));
  return JAT_OK;
}

int jat_rate_track(const uint8_t* cls, int32_t B, int32_t F, int32_t T, const float* rates, int32_t smooth, float* r,
                   void* stream) {
  JCHK(check_batch("jat_rate_track", B));
  if (F < 1) return fail(JAT_E_INVALID, "jat_rate_track: %d class frames, must be at least 1", F);
  if (T < 1) return fail(JAT_E_INVALID, "jat_rate_track: T %d must be at least 1", T);
  if (smooth < 0 || smooth > JAT_RATE_MAX_SMOOTH)
    return fail(JAT_E_INVALID, "jat_rate_track: smooth %d outside 0..%d", smooth, JAT_RATE_MAX_SMOOTH);
  if (!cls || !rates || !r) return fail(JAT_E_INVALID, "jat_rate_track: null buffer");
  float tb[3];
  for (int i = 0; i < 3; ++i) {
    if (!(rates[i] >= 0.f && rates[i] <= 1.f))                         // a NaN is outside
      return fail(JAT_E_INVALID, "jat_rate_track: rate %g of class %d outside [0, 1]", (double)rates[i], i);
    tb[i] = rates[i] + 0.f;                                            // -0 -> +0
  }
  KCHK(rate_track_launch(cls, B, F, T, tb[0], tb[1], tb[2], smooth, r, (hipStream_t)stream));
  return JAT_OK;
}

int jat_rate_mix(const float* x, const float* v, const float* rates, float* y, int32_t B, int32_t C, int32_t T, void* stream) {
  JCHK(check_batch("jat_rate_mix", B));
  if (C < 1) return fail(JAT_E_INVALID, "jat_rate_mix: channels %d must be at least 1", C);
  if (T < 1) return fail(JAT_E_INVALID, "jat_rate_mix: T %d must be at least 1", T);
  if (!x || !v || !rates || !y) return fail(JAT_E_INVALID, "jat_rate_mix: null buffer");
  const uint64_t bytes = (uint64_t)B * (uint64_t)C * (uint64_t)T * sizeof(float);
  if ((y != x && overlap(y, bytes, x, bytes)) || (y != v && overlap(y, bytes, v, bytes)) ||
      overlap(y, bytes, rates, (uint64_t)B * (uint64_t)T * sizeof(float)))
    return fail(JAT_E_INVALID, "jat_rate_mix: y overlaps an input it is not equal to");
  KCHK(rate_mix_launch(x, v, rates, y, B, C, T, (hipStream_t)stream));
  return JAT_OK;
}

}  // extern "C"
