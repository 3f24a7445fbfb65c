// C ABI of the training-data entry points (include/jat_hip.h): argument checks and the launches of data.hip.
#include "jat_data_kernels.h"
#include "jat_internal.h"

namespace {
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
}  // namespace

extern "C" {

int jat_latent_gather(const void* const* hr_src, const void* const* lr_src, const int64_t* len, const int64_t* start,
                      const float* hr_mean, const float* hr_std, const float* lr_mean, const float* lr_std, float* hr_out,
                      float* lr_out, int32_t B, int32_t C, int32_t T, void* stream) {
  if (!hr_src || !lr_src || !len || !start || !hr_out || !lr_out) return fail(JAT_E_INVALID, "jat_latent_gather: null buffer");
  if (B < 1 || C < 1 || T < 1) return fail(JAT_E_INVALID, "jat_latent_gather: B %d, C %d, T %d must be positive", B, C, T);
  if (T > DT_MAX_FRAMES) return fail(JAT_E_INVALID, "jat_latent_gather: T %d above %d", T, DT_MAX_FRAMES);
  if ((int64_t)B * C > 0x3fffffff) return fail(JAT_E_INVALID, "jat_latent_gather: %d x %d rows do not fit the grid", B, C);
  const int given = (hr_mean != nullptr) + (hr_std != nullptr) + (lr_mean != nullptr) + (lr_std != nullptr);
  if (given != 0 && given != 4)
    return fail(JAT_E_INVALID, "jat_latent_gather: the four statistics vectors are all given or all null");
  if (!aligned16(hr_out) || !aligned16(lr_out)) return fail(JAT_E_INVALID, "jat_latent_gather: outputs must be 16-byte aligned");
  KCHK(latent_gather_launch(hr_src, lr_src, len, start, hr_mean, hr_std, lr_mean, lr_std, hr_out, lr_out, B, C, T,
                            (hipStream_t)stream));
  return JAT_OK;
}

int jat_train_monitor(const float* pred, const float* target, const float* cond_clean, int64_t n, double* out, void* work,
                      size_t work_bytes, void* stream) {
  if (!pred || !target || !out || !work) return fail(JAT_E_INVALID, "jat_train_monitor: null buffer");
  if (n < 1) return fail(JAT_E_INVALID, "jat_train_monitor: n %lld must be at least 1", (long long)n);
  if (!aligned16(pred) || !aligned16(target) || !aligned16(cond_clean))
    return fail(JAT_E_INVALID, "jat_train_monitor: inputs must be 16-byte aligned");
  if (((uintptr_t)work & 7) || ((uintptr_t)out & 7)) return fail(JAT_E_INVALID, "jat_train_monitor: work and out must be 8-byte aligned");
  if (work_bytes < JAT_MONITOR_WORK_BYTES)
    return fail(JAT_E_STATE, "jat_train_monitor: workspace %zu < %d bytes", work_bytes, JAT_MONITOR_WORK_BYTES);
  static_assert(JAT_MONITOR_WORK_BYTES == MON_BLOCKS * MON_SUMS * sizeof(double), "header and kernel disagree");
  KCHK(train_monitor_launch(pred, target, cond_clean, n, (double*)work, out, (hipStream_t)stream));
  return JAT_OK;
}

}  // extern "C"
