// C ABI of the harmonic analysis, the harmonic template and the harmonic comparison (include/jat_hip_harm.h): the argument
// checks and the launches of harmonic.hip.  Stateless: the window is made inside the kernel, the scan's workspace is the caller's.
#include <cmath>

#include "../../include/jat_hip_harm.h"
#include "jat_harmonic_kernels.h"
#include "jat_internal.h"

namespace {

constexpr int64_t kMax31 = 0x7fffffff;

// the checks every entry shares: the [B, frames, H] table, then (analysis and synthesis) the framing of a row of L samples
int check_table(const char* who, int32_t B, int64_t frames, int32_t H) {
  if (B < 1 || B > 65535) return fail(JAT_E_INVALID, "%s: batch %d outside 1..65535", who, B);
  if (H < 1 || H > JAT_HARM_MAX) return fail(JAT_E_INVALID, "%s: n_harmonics %d outside 1..%d", who, H, JAT_HARM_MAX);
  if (frames < 1) return fail(JAT_E_INVALID, "%s: %lld frames, must be at least 1", who, (long long)frames);
  if (frames > kMax31 || frames * H > kMax31)
    return fail(JAT_E_INVALID, "%s: %lld frames x %d harmonics do not fit 31 bits", who, (long long)frames, H);
  return JAT_OK;
}

int check_framing(const char* who, int64_t L, int32_t hop, int32_t sr, int32_t frames) {
  if (sr < 1) return fail(JAT_E_INVALID, "%s: sample rate %d must be positive", who, sr);
  if (hop < 1) return fail(JAT_E_INVALID, "%s: hop_length %d must be at least 1", who, hop);
  if (L < 1) return fail(JAT_E_INVALID, "%s: length %lld must be at least 1", who, (long long)L);
  const int64_t want = 1 + L / hop;
  if (want > kMax31) return fail(JAT_E_INVALID, "%s: %lld frames do not fit 31 bits", who, (long long)want);
  if (frames != want)
    return fail(JAT_E_INVALID, "%s: %d frames, but length %lld at hop_length %d has 1 + L / hop = %lld", who, frames, (long long)L,
                hop, (long long)want);
  return JAT_OK;
}

}  // namespace

extern "C" {

int jat_harmonic_analyze(const float* x, int32_t B, int64_t L, const float* f0, const uint8_t* voiced, int32_t frames,
                         int32_t n_harmonics, int32_t sr, int32_t frame_length, int32_t hop_length, float* amp, float* energy,
                         void* stream) {
  const char* who = "harmonic_analyze";
  if (frame_length < 16 || frame_length > 8192 || (frame_length & 1))
    return fail(JAT_E_INVALID, "%s: frame_length %d must be even and in 16..8192", who, frame_length);
  JCHK(check_framing(who, L, hop_length, sr, frames));
  JCHK(check_table(who, B, frames, n_harmonics));
  if (!x || !f0 || !voiced || !amp) return fail(JAT_E_INVALID, "jat_harmonic_analyze: null buffer");
  HarmPlan p;
  p.N = frame_length, p.hop = hop_length, p.H = n_harmonics, p.sr = (double)sr;
  p.limit = (double)sr / 2.0 - 2.0 * (double)sr / (double)frame_length;
  KCHK(harm_analyze_launch(p, x, B, L, f0, voiced, frames, amp, energy, (hipStream_t)stream));
  return JAT_OK;
}

int jat_harmonic_synth_workspace_bytes(int32_t B, int64_t L, int32_t hop_length, size_t* bytes) {
  const char* who = "harmonic_synth_workspace_bytes";
  if (!bytes) return fail(JAT_E_INVALID, "jat_harmonic_synth_workspace_bytes: null output pointer");
  if (hop_length < 1) return fail(JAT_E_INVALID, "%s: hop_length %d must be at least 1", who, hop_length);
  if (L < 1) return fail(JAT_E_INVALID, "%s: length %lld must be at least 1", who, (long long)L);
  JCHK(check_table(who, B, 1 + L / hop_length, 1));
  *bytes = (size_t)B * (size_t)(1 + L / hop_length) * sizeof(uint32_t);
  return JAT_OK;
}

int jat_harmonic_synth(const float* f0, const uint8_t* voiced, const float* amp, int32_t B, int32_t frames,
                       int32_t n_harmonics, int64_t L, int32_t sr, int32_t hop_length, float* y, uint32_t* phase,
                       void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "harmonic_synth";
  JCHK(check_framing(who, L, hop_length, sr, frames));
  JCHK(check_table(who, B, frames, n_harmonics));
  if (!f0 || !voiced || !amp || !y) return fail(JAT_E_INVALID, "jat_harmonic_synth: null buffer");
  const size_t need = (size_t)B * (size_t)frames * sizeof(uint32_t);
  if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 3))
    return fail(JAT_E_INVALID, "%s: the workspace must be 4-byte aligned and hold %zu bytes, got %zu", who, need,
                workspace ? workspace_bytes : (size_t)0);
  HarmPlan p;
  p.hop = hop_length, p.H = n_harmonics, p.sr = (double)sr, p.limit = (double)sr / 2.0;
  KCHK(harm_synth_launch(p, f0, voiced, amp, B, frames, L, y, phase, (uint32_t*)workspace, (hipStream_t)stream));
  return JAT_OK;
}

int jat_harmonic_compare(const float* amp_a, const float* amp_ref, const float* f0_ref, const uint8_t* voiced_ref, int32_t B,
                         int32_t frames, int32_t n_harmonics, double cutoff_hz, double floor, double* out, void* stream) {
  const char* who = "harmonic_compare";
  JCHK(check_table(who, B, frames, n_harmonics));
  if (!(cutoff_hz >= 0.0)) return fail(JAT_E_INVALID, "%s: cutoff_hz %g must not be negative", who, cutoff_hz);
  if (!(floor > 0.0) || !std::isfinite(floor)) return fail(JAT_E_INVALID, "%s: floor %g must be positive and finite", who, floor);
  if (!amp_a || !amp_ref || !f0_ref || !voiced_ref || !out) return fail(JAT_E_INVALID, "jat_harmonic_compare: null buffer");
  KCHK(harm_compare_launch(amp_a, amp_ref, f0_ref, voiced_ref, B, frames, n_harmonics, cutoff_hz, floor, out,
                           (hipStream_t)stream));
  return JAT_OK;
}

}  // extern "C"
