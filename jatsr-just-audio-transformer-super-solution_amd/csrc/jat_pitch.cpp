// C ABI of the pitch tracker and the F0 comparison (include/jat_hip.h): the argument checks, the period range, the launches
// of pitch.hip.  Stateless: YIN needs no tables.
#include <cmath>

#include "jat_internal.h"
#include "jat_pitch_kernels.h"

namespace {

constexpr int64_t kMax31 = 0x7fffffff;

int check_range(int sr, double fmin, double fmax, int frame_length, int* min_period, int* max_period) {
  if (sr < 1) return fail(JAT_E_INVALID, "yin: sample rate %d must be positive", sr);
  if (frame_length < 16 || frame_length > 8192 || (frame_length & 1))
    return fail(JAT_E_INVALID, "yin: frame_length %d must be even and in 16..8192", frame_length);
  if (!(fmin > 0.0) || !std::isfinite(fmin)) return fail(JAT_E_INVALID, "yin: fmin %g must be positive", fmin);
  if (!(fmax > fmin) || !std::isfinite(fmax)) return fail(JAT_E_INVALID, "yin: fmax %g must be above fmin %g", fmax, fmin);
  if (!(fmax < sr / 2.0)) return fail(JAT_E_INVALID, "yin: fmax %g must be below sr / 2 = %g", fmax, sr / 2.0);
  const int W = frame_length / 2;
  const double lo = std::floor((double)sr / fmax), hi = std::fmin(std::ceil((double)sr / fmin), (double)(frame_length - W - 1));
  if (hi - lo < 2.0)
    return fail(JAT_E_INVALID, "yin: periods %g..%g (fmin %g, fmax %g, frame_length %d) leave fewer than 3 candidates", lo, hi,
                fmin, fmax, frame_length);
  *min_period = (int)lo, *max_period = (int)hi;
  return JAT_OK;
}

}  // namespace

extern "C" {

int jat_yin_periods(int32_t sr, double fmin, double fmax, int32_t frame_length, int32_t* min_period, int32_t* max_period) {
  if (!min_period || !max_period) return fail(JAT_E_INVALID, "jat_yin_periods: null output pointer");
  int lo = 0, hi = 0;
  JCHK(check_range(sr, fmin, fmax, frame_length, &lo, &hi));
  *min_period = lo, *max_period = hi;
  return JAT_OK;
}

int jat_yin(const jat_yin_params* params, const float* x, int32_t B, int64_t L, float* f0, float* aperiodicity, uint8_t* voiced,
            int32_t* index, float* d, float* cmndf, void* stream) {
  if (!params) return fail(JAT_E_INVALID, "jat_yin: null parameters");
  YinPlan p;
  JCHK(check_range(params->sr, params->fmin, params->fmax, params->frame_length, &p.min_period, &p.max_period));
  if (params->hop_length < 1) return fail(JAT_E_INVALID, "yin: hop_length %d must be at least 1", params->hop_length);
  if (!std::isfinite(params->trough_threshold)) return fail(JAT_E_INVALID, "yin: trough_threshold must be finite");
  if (B < 1 || B > 65535) return fail(JAT_E_INVALID, "yin: batch %d outside 1..65535", B);
  if (L < 1) return fail(JAT_E_INVALID, "yin: length %lld must be at least 1", (long long)L);
  const int64_t frames = 1 + L / params->hop_length;
  if (frames > kMax31) return fail(JAT_E_INVALID, "yin: %lld frames do not fit 31 bits", (long long)frames);
  if (frames * (p.max_period + 1) > kMax31)
    return fail(JAT_E_INVALID, "yin: %lld frames x %d lags do not fit 31 bits", (long long)frames, p.max_period + 1);
  if (!x || !f0 || !aperiodicity || !voiced) return fail(JAT_E_INVALID, "jat_yin: null buffer");
  p.frame_length = params->frame_length, p.hop = params->hop_length, p.W = params->frame_length / 2;
  p.sr = (float)params->sr, p.threshold = params->trough_threshold;
  KCHK(yin_launch(p, x, B, L, (int)frames, f0, aperiodicity, voiced, index, d, cmndf, (hipStream_t)stream));
  return JAT_OK;
}

int jat_f0_compare(const float* f0_a, const uint8_t* voiced_a, const float* f0_b, const uint8_t* voiced_b, int32_t B,
                   int32_t frames, double gross_cents, double* out, void* stream) {
  if (B < 1 || B > 65535) return fail(JAT_E_INVALID, "f0_compare: batch %d outside 1..65535", B);
  if (frames < 1) return fail(JAT_E_INVALID, "f0_compare: %d frames, must be at least 1", frames);
  if (!(gross_cents >= 0.0) || !std::isfinite(gross_cents))
    return fail(JAT_E_INVALID, "f0_compare: gross_cents %g must be finite and not negative", gross_cents);
  if (!f0_a || !voiced_a || !f0_b || !voiced_b || !out) return fail(JAT_E_INVALID, "jat_f0_compare: null buffer");
  KCHK(f0_compare_launch(f0_a, voiced_a, f0_b, voiced_b, B, frames, gross_cents, out, (hipStream_t)stream));
  return JAT_OK;
}

}  // extern "C"
