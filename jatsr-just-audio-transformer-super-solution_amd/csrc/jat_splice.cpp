// C ABI of the inverse STFT, the long-term spectrum and the low-band splice (include/jat_hip.h): the band gain and the
// overlap-add envelope in fp64 on the host, the argument checks, the launches of splice.hip.  The entry points hang on the
// jat_audio_metrics handle, which owns window, twiddles and envelope for its (n_fft, hop).
#include <cmath>

#include "jat_internal.h"
#include "jat_splice_kernels.h"

namespace {

constexpr int64_t kMax31 = 0x7fffffff;
constexpr double kPi = 3.14159265358979323846;

int check_transform(const char* who, int n_fft, int hop) {
  if (n_fft < 64 || n_fft > 4096 || (n_fft & (n_fft - 1)))
    return fail(JAT_E_INVALID, "%s: n_fft %d must be a power of two in 64..4096", who, n_fft);
  if (hop < 1 || n_fft % hop != 0) return fail(JAT_E_INVALID, "%s: hop %d must divide n_fft %d", who, hop, n_fft);
  if (hop > n_fft / 4) return fail(JAT_E_INVALID, "%s: hop %d must be at most n_fft / 4 = %d", who, hop, n_fft / 4);
  if (n_fft / hop > SP_MAX_OVERLAP)
    return fail(JAT_E_INVALID, "%s: overlap n_fft / hop = %d must be at most %d", who, n_fft / hop, SP_MAX_OVERLAP);
  return JAT_OK;
}

// B, the length and the frame count; the frames workspace [B, frames, n_fft] in bytes
int check_rows(const char* who, int n_fft, int hop, int32_t B, int64_t L, int* frames, size_t* bytes) {
  if (B < 1 || B > 65535) return fail(JAT_E_INVALID, "%s: batch %d outside 1..65535", who, B);
  if (L < 1) return fail(JAT_E_INVALID, "%s: length %lld must be at least 1", who, (long long)L);
  if (L + n_fft > kMax31) return fail(JAT_E_INVALID, "%s: length %lld does not fit 31 bits", who, (long long)L);
  const int64_t f = 1 + L / hop;
  if (f * (1 + n_fft / 2) > kMax31)
    return fail(JAT_E_INVALID, "%s: %lld frames x %d bins do not fit 31 bits", who, (long long)f, 1 + n_fft / 2);
  *frames = (int)f;
  *bytes = align_up((size_t)B * (size_t)f * n_fft * sizeof(float), 256);
  return JAT_OK;
}

int check_handle(const char* who, const jat_audio_metrics* h) {
  if (!h) return fail(JAT_E_INVALID, "%s: null handle", who);
  JCHK(check_transform(who, h->plan.n_fft, h->plan.hop));
  if (!h->envelope) return fail(JAT_E_STATE, "%s: the handle holds no envelope table", who);
  return JAT_OK;
}

}  // namespace

void splice_envelope_table(int n_fft, int hop, std::vector<float>* table) {
  const int R = n_fft / hop;
  std::vector<double> w2(n_fft);
  for (int i = 0; i < n_fft; ++i) {
    const double w = 0.5 - 0.5 * std::cos(2.0 * kPi * i / n_fft);
    w2[i] = w * w;
  }
  table->assign((size_t)R * (R + 1) / 2 * hop, 0.f);
  for (int m_hi = 0; m_hi < R; ++m_hi)
    for (int m_lo = 0; m_lo <= m_hi; ++m_lo)
      for (int r = 0; r < hop; ++r) {
        double s = 0.0;
        for (int m = m_hi; m >= m_lo; --m) s += w2[r + m * hop];   // frames ascending, as the kernel adds them
        (*table)[((size_t)m_hi * (m_hi + 1) / 2 + m_lo) * hop + r] = (float)s;
      }
}

extern "C" {

int jat_band_gain(int32_t sr, int32_t n_fft, double cutoff_hz, double transition_hz, float* a) {
  if (sr < 1) return fail(JAT_E_INVALID, "jat_band_gain: sample rate %d must be positive", sr);
  if (n_fft < 64 || n_fft > 4096 || (n_fft & (n_fft - 1)))
    return fail(JAT_E_INVALID, "jat_band_gain: n_fft %d must be a power of two in 64..4096", n_fft);
  if (!(transition_hz >= 0.0) || !std::isfinite(transition_hz) || !std::isfinite(cutoff_hz))
    return fail(JAT_E_INVALID, "jat_band_gain: cutoff %g Hz and transition %g Hz must be finite, the transition not negative",
                cutoff_hz, transition_hz);
  if (!a) return fail(JAT_E_INVALID, "jat_band_gain: null output pointer");
  const double lo = cutoff_hz - transition_hz;
  for (int k = 0; k <= n_fft / 2; ++k) {
    const double f = (double)k * (double)sr / (double)n_fft;
    a[k] = f >= cutoff_hz ? 0.f : (f <= lo ? 1.f : (float)(0.5 + 0.5 * std::cos(kPi * (f - lo) / transition_hz)));
  }
  return JAT_OK;
}

int jat_istft_workspace_bytes(int32_t n_fft, int32_t hop, int32_t B, int64_t L, size_t* bytes) {
  if (!bytes) return fail(JAT_E_INVALID, "jat_istft_workspace_bytes: null output pointer");
  JCHK(check_transform("jat_istft", n_fft, hop));
  int frames = 0;
  return check_rows("jat_istft", n_fft, hop, B, L, &frames, bytes);
}

int jat_istft(jat_audio_metrics* h, const void* X, int32_t B, int64_t L, float* y, void* work, size_t work_bytes, void* stream) {
  JCHK(check_handle("jat_istft", h));
  int frames = 0;
  size_t need = 0;
  JCHK(check_rows("jat_istft", h->plan.n_fft, h->plan.hop, B, L, &frames, &need));
  if (!X || !y || !work) return fail(JAT_E_INVALID, "jat_istft: null buffer");
  if (work_bytes < need) return fail(JAT_E_STATE, "jat_istft: workspace %zu < %zu bytes", work_bytes, need);
  hipStream_t s = (hipStream_t)stream;
  KCHK(istft_frames_launch(h->plan, h->tab, h->splice_slots, (const float2*)X, B, frames, (float*)work, s));
  KCHK(overlap_add_launch(h->plan, (const float*)work, h->envelope, B, frames, (int)L, nullptr, L, y, s));
  return JAT_OK;
}

int jat_ltas(jat_audio_metrics* h, const float* x, int32_t B, int64_t L, double* P, void* work, size_t work_bytes, void* stream) {
  if (!h) return fail(JAT_E_INVALID, "jat_ltas: null handle");
  if (h->plan.hop > h->plan.n_fft)
    return fail(JAT_E_INVALID, "jat_ltas: hop %d must be at most n_fft %d", h->plan.hop, h->plan.n_fft);
  int frames = 0;
  size_t unused = 0;
  JCHK(check_rows("jat_ltas", h->plan.n_fft, h->plan.hop, B, L, &frames, &unused));
  if (!x || !P || !work) return fail(JAT_E_INVALID, "jat_ltas: null buffer");
  const size_t need = (size_t)B * LT_SLICES * h->plan.bins * sizeof(double);
  if (work_bytes < need) return fail(JAT_E_STATE, "jat_ltas: workspace %zu < %zu bytes", work_bytes, need);
  KCHK(ltas_launch(h->plan, h->tab, x, B, (int)L, frames, (double*)work, P, (hipStream_t)stream));
  return JAT_OK;
}

int jat_band_splice_workspace_bytes(int32_t n_fft, int32_t hop, int32_t B, int64_t L_gen, int64_t L_src, size_t* bytes) {
  if (!bytes) return fail(JAT_E_INVALID, "jat_band_splice_workspace_bytes: null output pointer");
  JCHK(check_transform("jat_band_splice", n_fft, hop));
  if (L_gen < 1 || L_src < 1)
    return fail(JAT_E_INVALID, "jat_band_splice: lengths %lld and %lld must be at least 1", (long long)L_gen, (long long)L_src);
  int frames = 0;
  JCHK(check_rows("jat_band_splice", n_fft, hop, B, L_gen, &frames, bytes));   // the 31-bit check on the full length
  return check_rows("jat_band_splice", n_fft, hop, B, L_gen < L_src ? L_gen : L_src, &frames, bytes);
}

int jat_band_splice(jat_audio_metrics* h, const float* generated, const float* source, int32_t B, int64_t L_gen, int64_t L_src,
                    const float* a, float* out, void* work, size_t work_bytes, void* stream) {
  JCHK(check_handle("jat_band_splice", h));
  size_t need = 0;
  JCHK(jat_band_splice_workspace_bytes(h->plan.n_fft, h->plan.hop, B, L_gen, L_src, &need));
  if (!generated || !source || !a || !out || !work) return fail(JAT_E_INVALID, "jat_band_splice: null buffer");
  if (work_bytes < need) return fail(JAT_E_STATE, "jat_band_splice: workspace %zu < %zu bytes", work_bytes, need);
  const int n = (int)(L_gen < L_src ? L_gen : L_src), frames = 1 + n / h->plan.hop;
  hipStream_t s = (hipStream_t)stream;
  KCHK(splice_frames_launch(h->plan, h->tab, h->splice_slots, generated, source, B, L_gen, L_src, n, frames, a, (float*)work, s));
  KCHK(overlap_add_launch(h->plan, (const float*)work, h->envelope, B, frames, n, generated, L_gen, out, s));
  return JAT_OK;
}

}  // extern "C"
