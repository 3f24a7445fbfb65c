// C ABI of the audio-quality metrics (include/jat_hip.h): the Slaney mel filterbank, the Hann window and the per-pass
// twiddle tables in fp64 on the host, the metrics handle (which also carries the tables of jat_splice.cpp), the launches of
// metrics.hip.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "jat_internal.h"
#include "jat_metrics_kernels.h"
#include "jat_splice_kernels.h"

namespace {

constexpr int64_t kMax31 = 0x7fffffff;
constexpr double kPi = 3.14159265358979323846;

int check_sizes(int sr, int n_fft, int n_mels) {
  if (sr < 1) return fail(JAT_E_INVALID, "metrics: sample rate %d must be positive", sr);
  if (n_fft < 64 || n_fft > 4096 || (n_fft & (n_fft - 1)))
    return fail(JAT_E_INVALID, "metrics: n_fft %d must be a power of two in 64..4096", n_fft);
  if (n_mels < 0 || n_mels > 1 + n_fft / 2)
    return fail(JAT_E_INVALID, "metrics: n_mels %d outside 0..%d (the bin count)", n_mels, 1 + n_fft / 2);
  return JAT_OK;
}

// librosa's Slaney scale (htk=False): linear below 1 kHz at 200/3 Hz per mel, logarithmic above with ln(6.4)/27 per mel
double hz_to_mel(double f) {
  const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
  return f >= min_log_hz ? min_log_mel + std::log(f / min_log_hz) / logstep : f / f_sp;
}
double mel_to_hz(double m) {
  const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
  return m >= min_log_mel ? min_log_hz * std::exp(logstep * (m - min_log_mel)) : f_sp * m;
}

// librosa.filters.mel(sr, n_fft, n_mels): fmin 0, fmax sr / 2, norm="slaney"; fp64, stored as fp32; out [n_mels][bins]
void filterbank(int sr, int n_fft, int n_mels, float* out) {
  const int bins = 1 + n_fft / 2;
  std::vector<double> mel_f(n_mels + 2);
  const double m0 = hz_to_mel(0.0), m1 = hz_to_mel(sr / 2.0), step = (m1 - m0) / (n_mels + 1);
  for (int i = 0; i < n_mels + 2; ++i) mel_f[i] = mel_to_hz(i == n_mels + 1 ? m1 : m0 + i * step);
  for (int m = 0; m < n_mels; ++m) {
    const double lo = mel_f[m], ce = mel_f[m + 1], hi = mel_f[m + 2], enorm = 2.0 / (hi - lo);
    for (int k = 0; k < bins; ++k) {
      const double f = (double)k * ((double)sr / n_fft);
      const double lower = -(lo - f) / (ce - lo), upper = (hi - f) / (hi - ce);
      out[(size_t)m * bins + k] = (float)(std::max(0.0, std::min(lower, upper)) * enorm);
    }
  }
}

void make_plan(int n_fft, int hop, int n_mels, MetricsPlan* p, std::vector<float2>* tw) {
  p->n_fft = n_fft, p->hop = hop, p->bins = 1 + n_fft / 2, p->n_mels = n_mels;
  p->group = MT_GROUP_POINTS / n_fft < 1 ? 1 : MT_GROUP_POINTS / n_fft;
  p->n_pass = 0;
  tw->clear();
  int ns = 1;
  while (ns < n_fft) {
    const int R = ns * 4 <= n_fft ? 4 : 2, i = p->n_pass++;
    p->radix[i] = R, p->ns[i] = ns, p->off[i] = (int)tw->size();
    if (ns > 1) {             // the first pass has no twiddles
      for (int r = 1; r < R; ++r)
        for (int k = 0; k < ns; ++k) {
          const double a = -2.0 * kPi * (double)r * (double)k / ((double)ns * R);
          tw->push_back(make_float2((float)std::cos(a), (float)std::sin(a)));
        }
    }
    ns *= R;
  }
  p->n_tw = (int)tw->size();
}

int check_shape(const jat_audio_metrics* h, int32_t B, int64_t L, int* frames) {
  if (!h) return fail(JAT_E_INVALID, "metrics: null handle");
  if (B < 1 || B > 65535) return fail(JAT_E_INVALID, "metrics: batch %d outside 1..65535", B);
  if (L < 1) return fail(JAT_E_INVALID, "metrics: length %lld must be at least 1", (long long)L);
  if (L + h->plan.n_fft > kMax31) return fail(JAT_E_INVALID, "metrics: length %lld does not fit 31 bits", (long long)L);
  const int64_t f = 1 + L / h->plan.hop;
  if (f * h->plan.bins > kMax31)
    return fail(JAT_E_INVALID, "metrics: %lld frames x %d bins do not fit 31 bits", (long long)f, h->plan.bins);
  *frames = (int)f;
  return JAT_OK;
}

struct WorkLayout {
  size_t partial = 0, mel_pow = 0, block_max = 0, lsd_frames = 0, total = 0;
  int nbx = 0;
};
WorkLayout work_layout(const jat_audio_metrics* h, int B, int frames) {
  WorkLayout w;
  w.nbx = metrics_blocks_per_row(h->plan, B, frames);
  size_t o = 0;
  w.partial = o, o = align_up(o + (size_t)B * MT_SLICES * 3 * sizeof(double), 256);
  w.mel_pow = o, o = align_up(o + (size_t)B * 2 * frames * h->plan.n_mels * sizeof(float), 256);
  w.block_max = o, o = align_up(o + (size_t)B * 2 * w.nbx * sizeof(float), 256);
  w.lsd_frames = o, o = align_up(o + (size_t)B * frames * sizeof(float), 256);
  w.total = o;
  return w;
}

}  // namespace

extern "C" {

int jat_mel_filterbank(int32_t sr, int32_t n_fft, int32_t n_mels, float* out) {
  JCHK(check_sizes(sr, n_fft, n_mels));
  if (out && n_mels > 0) filterbank(sr, n_fft, n_mels, out);
  return JAT_OK;
}

int jat_stft_frames(int64_t L, int32_t hop, int64_t* frames) {
  if (!frames) return fail(JAT_E_INVALID, "jat_stft_frames: null output pointer");
  if (L < 1) return fail(JAT_E_INVALID, "metrics: length %lld must be at least 1", (long long)L);
  if (hop < 1) return fail(JAT_E_INVALID, "metrics: hop %d must be at least 1", hop);
  *frames = 1 + L / hop;
  return JAT_OK;
}

int jat_audio_metrics_create(int32_t sr, int32_t n_fft, int32_t hop, int32_t n_mels, void* stream, jat_audio_metrics** out) {
  if (!out) return fail(JAT_E_INVALID, "jat_audio_metrics_create: null output pointer");
  *out = nullptr;
  JCHK(check_sizes(sr, n_fft, n_mels));
  if (hop < 1) return fail(JAT_E_INVALID, "metrics: hop %d must be at least 1", hop);
  std::unique_ptr<jat_audio_metrics> h(new jat_audio_metrics);
  std::vector<float2> tw;
  make_plan(n_fft, hop, n_mels, &h->plan, &tw);
  const int bins = h->plan.bins;
  std::vector<float> window(n_fft);
  for (int i = 0; i < n_fft; ++i) window[i] = (float)(0.5 - 0.5 * std::cos(2.0 * kPi * i / n_fft));
  // the filterbank kept sparse: per band its first bin, its bin count and its weights
  std::vector<int> first(n_mels), count(n_mels), off(n_mels);
  std::vector<float> bw;
  if (n_mels > 0) {
    std::vector<float> dense((size_t)n_mels * bins);
    filterbank(sr, n_fft, n_mels, dense.data());
    for (int m = 0; m < n_mels; ++m) {
      const float* row = dense.data() + (size_t)m * bins;
      int a = 0, b = bins - 1;
      while (a < bins && !(row[a] > 0.f)) ++a;
      while (b >= a && !(row[b] > 0.f)) --b;
      first[m] = a < bins ? a : 0, count[m] = a < bins ? b - a + 1 : 0, off[m] = (int)bw.size();
      for (int k = 0; k < count[m]; ++k) bw.push_back(row[a + k]);
    }
  }
  if ((int)bw.size() > n_fft - 2)   // cannot happen: at most two triangles over a bin, none over the two edge bins
    return fail(JAT_E_STATE, "metrics: filterbank of %zu non-zeros for n_fft %d", bw.size(), n_fft);
  h->plan.nnz = (int)bw.size();
  {
    int dev = 0, cus = 0;
    HIPCHK(hipGetDevice(&dev));
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    int per_cu = 0;
    KCHK(metrics_blocks_per_cu(h->plan, &per_cu));
    h->plan.slots = cus * per_cu < 1 ? 1 : cus * per_cu;
    KCHK(splice_blocks_per_cu(h->plan, &per_cu));
    h->splice_slots = cus * per_cu < 1 ? 1 : cus * per_cu;
  }
  // the overlap-add envelope of the inverse transform, where hop allows one (jat_splice_kernels.h)
  std::vector<float> env;
  if (splice_hop_ok(n_fft, hop)) splice_envelope_table(n_fft, hop, &env);
  // one device allocation: twiddles, window, band tables, weights
  std::vector<char> host;
  auto put = [&](const void* p, size_t n) {
    const size_t at = align_up(host.size(), 16);
    host.resize(at + n);
    if (n) memcpy(host.data() + at, p, n);
    return at;
  };
  const size_t o_tw = put(tw.data(), tw.size() * sizeof(float2)), o_win = put(window.data(), window.size() * sizeof(float));
  const size_t o_first = put(first.data(), first.size() * sizeof(int)), o_count = put(count.data(), count.size() * sizeof(int));
  const size_t o_off = put(off.data(), off.size() * sizeof(int)), o_w = put(bw.data(), bw.size() * sizeof(float));
  const size_t o_env = put(env.data(), env.size() * sizeof(float));
  host.resize(align_up(host.size() + 16, 16));
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipMalloc(&h->dev, host.size()));
  hipError_t e = hipMemcpyAsync(h->dev, host.data(), host.size(), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);   // host leaves scope
  if (e != hipSuccess) {
    (void)hipFree(h->dev);
    return fail(JAT_E_HIP, "jat_audio_metrics_create: table upload failed: %s", hipGetErrorString(e));
  }
  char* d = (char*)h->dev;
  h->tab.tw = (const float2*)(d + o_tw), h->tab.window = (const float*)(d + o_win);
  h->tab.band_first = (const int*)(d + o_first), h->tab.band_count = (const int*)(d + o_count);
  h->tab.band_off = (const int*)(d + o_off), h->tab.band_w = (const float*)(d + o_w);
  h->envelope = env.empty() ? nullptr : (const float*)(d + o_env);
  *out = h.release();
  return JAT_OK;
}

void jat_audio_metrics_destroy(jat_audio_metrics* h) {
  if (!h) return;
  if (h->dev) (void)hipFree(h->dev);
  delete h;
}

int jat_audio_metrics_workspace_bytes(const jat_audio_metrics* h, int32_t B, int64_t L, size_t* bytes) {
  if (!bytes) return fail(JAT_E_INVALID, "jat_audio_metrics_workspace_bytes: null output pointer");
  int frames = 0;
  JCHK(check_shape(h, B, L, &frames));
  *bytes = work_layout(h, B, frames).total;
  return JAT_OK;
}

int jat_audio_metrics_run(jat_audio_metrics* h, const float* pred, const float* gt, int32_t B, int64_t L, int32_t want_lsd,
                          double* out, float* lsd_frames, float* pred_db, float* gt_db, void* work, size_t work_bytes,
                          void* stream) {
  int frames = 0;
  JCHK(check_shape(h, B, L, &frames));
  if (!pred || !gt || !out || !work) return fail(JAT_E_INVALID, "jat_audio_metrics_run: null buffer");
  if ((pred_db == nullptr) != (gt_db == nullptr) || (pred_db && h->plan.n_mels == 0))
    return fail(JAT_E_INVALID, "jat_audio_metrics_run: pred_db and gt_db go together and need a handle with mel bands");
  if (lsd_frames && !want_lsd) return fail(JAT_E_INVALID, "jat_audio_metrics_run: lsd_frames given without want_lsd");
  const WorkLayout w = work_layout(h, B, frames);
  if (work_bytes < w.total) return fail(JAT_E_STATE, "jat_audio_metrics_run: workspace %zu < %zu bytes", work_bytes, w.total);
  char* base = (char*)work;
  float* mel_pow = h->plan.n_mels > 0 ? (float*)(base + w.mel_pow) : nullptr;
  float* block_max = mel_pow ? (float*)(base + w.block_max) : nullptr;
  float* lf = want_lsd ? (lsd_frames ? lsd_frames : (float*)(base + w.lsd_frames)) : nullptr;
  hipStream_t s = (hipStream_t)stream;
  KCHK(metrics_stft_launch(h->plan, h->tab, pred, gt, B, (int)L, frames, mel_pow, block_max, lf, nullptr, nullptr, s));
  KCHK(metrics_finish_launch(h->plan, mel_pow, block_max, w.nbx, lf, B, frames, (double*)(base + w.partial), out, pred_db,
                             gt_db, s));
  return JAT_OK;
}

int jat_stft(jat_audio_metrics* h, const float* x, const float* y, int32_t B, int64_t L, void* X, void* Y, void* stream) {
  int frames = 0;
  JCHK(check_shape(h, B, L, &frames));
  if (!x || !X) return fail(JAT_E_INVALID, "jat_stft: null buffer");
  if ((y == nullptr) != (Y == nullptr)) return fail(JAT_E_INVALID, "jat_stft: y and Y go together");
  KCHK(metrics_stft_launch(h->plan, h->tab, x, y ? y : x, B, (int)L, frames, nullptr, nullptr, nullptr, (float2*)X, (float2*)Y,
                           (hipStream_t)stream));
  return JAT_OK;
}

}  // extern "C"
