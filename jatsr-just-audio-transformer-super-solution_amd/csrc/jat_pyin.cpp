// C ABI of the pYIN tracker (include/jat_hip.h): the argument checks, the host-made tables (threshold prior, Boltzmann
// weights, transition weights, pitch bins), the workspace layout and the launches of pitch.hip (the difference function) and
// pyin.hip.  The tables are made in fp64 and rounded once; they reach the device at the first jat_pyin_track, so that
// creating a handle and reading its tables need no GPU.
#include <cfloat>
#include <cmath>

#include "jat_internal.h"
#include "jat_pitch_kernels.h"
#include "jat_pyin_kernels.h"

struct jat_pyin {
  jat_pyin_params par;
  YinPlan yin;
  PyinPlan plan;
  std::vector<double> beta;                       // [N]
  std::vector<float> theta, beta32, cum_beta, A, invD, logw, logZ, freqs;
  float* dev = nullptr;                           // one allocation holding the eight device tables
  int device = -1;                                // the device that holds them: the one current at the first track
  bool profile = false;
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
};

namespace {

constexpr int64_t kMax31 = 0x7fffffff;

// I_x(a, b) by the continued fraction of the incomplete beta function (modified Lentz), fp64
double betainc(double a, double b, double x) {
  if (x <= 0.0) return 0.0;
  if (x >= 1.0) return 1.0;
  if (x > (a + 1.0) / (a + b + 2.0)) return 1.0 - betainc(b, a, 1.0 - x);
  const double front = std::exp(std::lgamma(a + b) - std::lgamma(a) - std::lgamma(b) + a * std::log(x) + b * std::log1p(-x)) / a;
  const double tiny = 1e-300;
  double c = 1.0, d = 1.0 - (a + b) * x / (a + 1.0);
  d = 1.0 / (std::fabs(d) > tiny ? d : tiny);
  double f = d;
  for (int m = 1; m < 1000; ++m) {
    const double num[2] = {m * (b - m) * x / ((a + 2 * m - 1) * (a + 2 * m)),
                           -(a + m) * (a + b + m) * x / ((a + 2 * m) * (a + 2 * m + 1))};
    double step = 1.0;
    for (int q = 0; q < 2; ++q) {
      d = 1.0 + num[q] * d;
      d = 1.0 / (std::fabs(d) > tiny ? d : tiny);
      c = 1.0 + num[q] / c;
      c = std::fabs(c) > tiny ? c : tiny;
      step = d * c;
      f *= step;
    }
    if (std::fabs(step - 1.0) < 1e-16) break;
  }
  return front * f;
}

bool positive(double v) { return std::isfinite(v) && v > 0.0; }
bool probability(double v) { return std::isfinite(v) && v > 0.0 && v < 1.0; }

struct Layout {
  size_t f0, ap, voiced, cmndf, log_obs, back, state, total;
};
Layout layout(const jat_pyin* h, int64_t B, int64_t frames) {
  const size_t n = (size_t)B * (size_t)frames, nb = (size_t)h->plan.n_bins;
  Layout l;
  size_t at = 0;
  auto take = [&](size_t bytes) { const size_t o = at; at = align_up(at + bytes, 256); return o; };
  l.f0 = take(n * 4), l.ap = take(n * 4), l.voiced = take(n), l.cmndf = take(n * (size_t)h->plan.lags * 4);
  l.log_obs = take(n * (nb + 1) * 4), l.back = take(n * 2 * nb * 2), l.state = take(n * 4);
  l.total = at;
  return l;
}

int check_shape(const jat_pyin* h, int32_t B, int64_t L, int64_t* frames) {
  if (!h) return fail(JAT_E_INVALID, "pyin: null handle");
  if (B < 1 || B > 65535) return fail(JAT_E_INVALID, "pyin: batch %d outside 1..65535", B);
  if (L < 1) return fail(JAT_E_INVALID, "pyin: length %lld must be at least 1", (long long)L);
  const int64_t f = 1 + L / h->par.hop_length;
  const int64_t widest = std::max<int64_t>(std::max<int64_t>(h->plan.lags, 2 * (int64_t)h->plan.n_bins), h->plan.n_bins + 1);
  if (f > kMax31 || f * widest > kMax31)
    return fail(JAT_E_INVALID, "pyin: %lld frames x %lld values per frame do not fit 31 bits", (long long)f, (long long)widest);
  *frames = f;
  return JAT_OK;
}

int upload(jat_pyin* h) {
  int cur = -1;
  HIPCHK(hipGetDevice(&cur));
  if (h->dev) {
    if (cur != h->device)
      return fail(JAT_E_STATE, "pyin: the handle's tables are on device %d, the current device is %d; a handle serves one device",
                  h->device, cur);
    return JAT_OK;
  }
  const std::vector<float>* t[8] = {&h->theta, &h->beta32, &h->cum_beta, &h->A, &h->invD, &h->logw, &h->logZ, &h->freqs};
  std::vector<float> all;
  size_t off[8];
  for (int i = 0; i < 8; ++i) {
    off[i] = all.size();
    all.insert(all.end(), t[i]->begin(), t[i]->end());
    all.resize(align_up(all.size(), 4), 0.f);
  }
  float* d = nullptr;
  HIPCHK(hipMalloc(&d, all.size() * sizeof(float)));
  hipError_t e = hipMemcpy(d, all.data(), all.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(d);
    return fail(JAT_E_HIP, "pyin: table upload failed: %s", hipGetErrorString(e));
  }
  h->dev = d, h->device = cur;
  PyinPlan& p = h->plan;
  p.theta = d + off[0], p.beta = d + off[1], p.cum_beta = d + off[2], p.A = d + off[3], p.invD = d + off[4];
  p.logw = d + off[5], p.logZ = d + off[6], p.freqs = d + off[7];
  return JAT_OK;
}

}  // namespace

extern "C" {

int jat_pyin_beta_probs(double a, double b, int32_t n, double* out) {
  if (!out) return fail(JAT_E_INVALID, "jat_pyin_beta_probs: null output pointer");
  if (!positive(a) || !positive(b)) return fail(JAT_E_INVALID, "pyin: beta parameters (%g, %g) must be positive and finite", a, b);
  if (n < 1 || n > 65536) return fail(JAT_E_INVALID, "pyin: %d thresholds outside 1..65536", n);
  double before = 0.0;
  for (int m = 1; m <= n; ++m) {
    const double cdf = m == n ? 1.0 : betainc(a, b, (double)m / n);
    out[m - 1] = cdf > before ? cdf - before : 0.0;          // a mass is never negative
    before = cdf;
  }
  return JAT_OK;
}

int jat_pyin_create(const jat_pyin_params* par, jat_pyin** out) {
  if (!par || !out) return fail(JAT_E_INVALID, "jat_pyin_create: null pointer");
  int lo = 0, hi = 0;
  JCHK(jat_yin_periods(par->sr, par->fmin, par->fmax, par->frame_length, &lo, &hi));
  if (par->hop_length < 1) return fail(JAT_E_INVALID, "pyin: hop_length %d must be at least 1", par->hop_length);
  if (par->n_thresholds < 1 || par->n_thresholds > PY_MAX_THRESHOLDS)
    return fail(JAT_E_INVALID, "pyin: n_thresholds %d outside 1..%d", par->n_thresholds, PY_MAX_THRESHOLDS);
  if (!positive(par->beta_a) || !positive(par->beta_b))
    return fail(JAT_E_INVALID, "pyin: beta_parameters (%g, %g) must be positive and finite", par->beta_a, par->beta_b);
  if (!positive(par->boltzmann_parameter))
    return fail(JAT_E_INVALID, "pyin: boltzmann_parameter %g must be positive and finite", par->boltzmann_parameter);
  if (!positive(par->max_transition_rate))
    return fail(JAT_E_INVALID, "pyin: max_transition_rate %g must be positive and finite", par->max_transition_rate);
  if (!probability(par->switch_prob)) return fail(JAT_E_INVALID, "pyin: switch_prob %g must lie inside (0, 1)", par->switch_prob);
  if (!probability(par->no_trough_prob))
    return fail(JAT_E_INVALID, "pyin: no_trough_prob %g must lie inside (0, 1)", par->no_trough_prob);
  if (!(par->resolution > 0.0 && par->resolution <= 1.0))
    return fail(JAT_E_INVALID, "pyin: resolution %g must lie inside (0, 1]", par->resolution);
  const double bps_d = std::ceil(1.0 / par->resolution);
  const double bins_d = bps_d <= 1e6 ? std::floor(12.0 * bps_d * std::log2(par->fmax / par->fmin)) + 1.0 : 1e300;
  if (!(bins_d >= 1.0 && bins_d <= (double)PY_MAX_BINS))
    return fail(JAT_E_INVALID, "pyin: %g pitch bins (resolution %g over %g..%g Hz); the kernels take 1..%d", bins_d, par->resolution,
                par->fmin, par->fmax, PY_MAX_BINS);
  const double H_d = std::nearbyint(par->max_transition_rate * 12 * par->hop_length / par->sr) * bps_d;
  if (!(H_d >= 0.0 && H_d <= (double)PY_MAX_H))
    return fail(JAT_E_INVALID, "pyin: a transition of %g bins a frame; the kernels take 0..%d", H_d, PY_MAX_H);
  const int ny = hi - lo + 1;
  if (ny > PY_MAX_NY) return fail(JAT_E_INVALID, "pyin: %d candidates a frame; the kernels take up to %d", ny, PY_MAX_NY);

  std::unique_ptr<jat_pyin> h(new jat_pyin);
  h->par = *par;
  const int N = par->n_thresholds, bps = (int)bps_d, nb = (int)bins_d, H = (int)H_d, ntm = ny / 2 + 1;
  const double lam = par->boltzmann_parameter;
  h->yin.frame_length = par->frame_length, h->yin.hop = par->hop_length, h->yin.W = par->frame_length / 2;
  h->yin.min_period = lo, h->yin.max_period = hi, h->yin.sr = (float)par->sr, h->yin.threshold = 0.1f;
  PyinPlan& p = h->plan;
  p.min_period = lo, p.ny = ny, p.lags = hi + 1, p.n_thresholds = N, p.n_bins = nb, p.H = H, p.nt_max = ntm;
  p.sr = (double)par->sr, p.fmin = par->fmin, p.bin_scale = 12.0 * bps;
  p.no_trough_prob = (float)par->no_trough_prob;
  p.lk = (float)std::log(1.0 - par->switch_prob), p.ls = (float)std::log(par->switch_prob), p.logpi = (float)std::log(1.0 / (2 * nb));

  h->beta.resize(N);
  JCHK(jat_pyin_beta_probs(par->beta_a, par->beta_b, N, h->beta.data()));
  h->theta.assign(N + 2, 0.f), h->beta32.assign(N + 1, 0.f), h->cum_beta.assign(N + 2, 0.f);
  h->theta[0] = -INFINITY, h->theta[N + 1] = INFINITY;
  double cum = 0.0;
  for (int m = 1; m <= N; ++m) {
    h->theta[m] = (float)((double)m / N);
    h->beta32[m] = (float)h->beta[m - 1];
    h->cum_beta[m] = (float)cum;                              // sum of beta_1 .. beta_(m - 1)
    cum += h->beta[m - 1];
  }
  h->cum_beta[N + 1] = (float)cum;
  h->A.assign(ntm + 1, 0.f), h->invD.assign(ntm + 1, 0.f);
  for (int k = 0; k <= ntm; ++k) {
    const double a = -std::expm1(-lam) * std::exp(-lam * k);
    h->A[k] = a < (double)FLT_MIN ? 0.f : (float)a;
    if (k >= 1) h->invD[k] = (float)(1.0 / -std::expm1(-lam * k));
  }
  h->logw.resize(2 * H + 1), h->logZ.resize(nb), h->freqs.resize(nb);
  std::vector<double> w(2 * H + 1);
  for (int j = 0; j <= 2 * H; ++j) {
    w[j] = 1.0 - std::abs(j - H) / (H + 1.0);
    h->logw[j] = (float)std::log(w[j]);
  }
  for (int r = 0; r < nb; ++r) {
    double Z = 0.0;
    for (int j = 0; j <= 2 * H; ++j)
      if (r + j - H >= 0 && r + j - H < nb) Z += w[j];
    h->logZ[r] = (float)std::log(Z);
    h->freqs[r] = (float)(par->fmin * std::pow(2.0, r / (12.0 * bps)));
  }
  *out = h.release();
  return JAT_OK;
}

void jat_pyin_destroy(jat_pyin* h) {
  if (!h) return;
  for (hipEvent_t e : h->ev)
    if (e) (void)hipEventDestroy(e);
  if (h->dev) (void)hipFree(h->dev);
  delete h;
}

int jat_pyin_shape(const jat_pyin* h, int32_t* n_bins, int32_t* H, int32_t* min_period, int32_t* max_period) {
  if (!h) return fail(JAT_E_INVALID, "jat_pyin_shape: null handle");
  if (n_bins) *n_bins = h->plan.n_bins;
  if (H) *H = h->plan.H;
  if (min_period) *min_period = h->plan.min_period;
  if (max_period) *max_period = h->plan.lags - 1;
  return JAT_OK;
}

int jat_pyin_tables(const jat_pyin* h, double* beta, float* logw, float* logZ, float* freqs, float* scalars) {
  if (!h) return fail(JAT_E_INVALID, "jat_pyin_tables: null handle");
  if (beta) std::copy(h->beta.begin(), h->beta.end(), beta);
  if (logw) std::copy(h->logw.begin(), h->logw.end(), logw);
  if (logZ) std::copy(h->logZ.begin(), h->logZ.end(), logZ);
  if (freqs) std::copy(h->freqs.begin(), h->freqs.end(), freqs);
  if (scalars) scalars[0] = h->plan.lk, scalars[1] = h->plan.ls, scalars[2] = h->plan.logpi;
  return JAT_OK;
}

int jat_pyin_workspace_bytes(const jat_pyin* h, int32_t B, int64_t L, size_t* bytes) {
  if (!bytes) return fail(JAT_E_INVALID, "jat_pyin_workspace_bytes: null output pointer");
  int64_t frames = 0;
  JCHK(check_shape(h, B, L, &frames));
  *bytes = layout(h, B, frames).total;
  return JAT_OK;
}

int jat_pyin_track(jat_pyin* h, const float* x, int32_t B, int64_t L, float* f0, uint8_t* voiced, float* voiced_prob, float* cmndf,
                   float* prob, int32_t* bin, float* obs, float* log_obs, int32_t* state, void* work, size_t work_bytes,
                   void* stream) {
  int64_t frames64 = 0;
  JCHK(check_shape(h, B, L, &frames64));
  if (!x || !f0 || !voiced || !voiced_prob || !work) return fail(JAT_E_INVALID, "jat_pyin_track: null buffer");
  if (((uintptr_t)work & 15) != 0) return fail(JAT_E_INVALID, "jat_pyin_track: the workspace must be 16-byte aligned");
  const Layout l = layout(h, B, frames64);
  if (work_bytes < l.total)
    return fail(JAT_E_STATE, "jat_pyin_track: workspace of %zu bytes, %zu needed", work_bytes, l.total);
  JCHK(upload(h));
  const int frames = (int)frames64;
  hipStream_t s = (hipStream_t)stream;
  char* wk = (char*)work;
  float* c = cmndf ? cmndf : (float*)(wk + l.cmndf);
  float* lo = log_obs ? log_obs : (float*)(wk + l.log_obs);
  int32_t* st = state ? state : (int32_t*)(wk + l.state);
  if (h->profile)
    for (hipEvent_t& e : h->ev)
      if (!e) HIPCHK(hipEventCreate(&e));
  auto mark = [&](int i) { return h->profile ? hipEventRecord(h->ev[i], s) : hipSuccess; };
  KCHK(mark(0));
  KCHK(yin_launch(h->yin, x, B, L, frames, (float*)(wk + l.f0), (float*)(wk + l.ap), (uint8_t*)(wk + l.voiced), nullptr, nullptr, c, s));
  KCHK(mark(1));
  KCHK(pyin_observe_launch(h->plan, c, B, frames, voiced_prob, lo, prob, bin, obs, s));
  KCHK(mark(2));
  KCHK(pyin_forward_launch(h->plan, lo, B, frames, (uint16_t*)(wk + l.back), st, s));
  KCHK(mark(3));
  KCHK(pyin_trace_launch(h->plan, B, frames, (const uint16_t*)(wk + l.back), st, f0, voiced, s));
  KCHK(mark(4));
  return JAT_OK;
}

int jat_pyin_decode(jat_pyin* h, const float* log_obs, int32_t B, int32_t frames, int32_t* state, float* f0, uint8_t* voiced,
                    void* work, size_t work_bytes, void* stream) {
  if (!h) return fail(JAT_E_INVALID, "jat_pyin_decode: null handle");
  if (B < 1 || B > 65535) return fail(JAT_E_INVALID, "pyin: batch %d outside 1..65535", B);
  if (frames < 1 || (int64_t)frames * (2 * (int64_t)h->plan.n_bins) > kMax31)
    return fail(JAT_E_INVALID, "pyin: %d frames x %d states must be at least 1 and fit 31 bits", frames, 2 * h->plan.n_bins);
  if (!log_obs || !state || !f0 || !voiced || !work) return fail(JAT_E_INVALID, "jat_pyin_decode: null buffer");
  if (((uintptr_t)work & 15) != 0) return fail(JAT_E_INVALID, "jat_pyin_decode: the workspace must be 16-byte aligned");
  const size_t need = (size_t)B * (size_t)frames * (size_t)h->plan.n_bins * 4;
  if (work_bytes < need) return fail(JAT_E_STATE, "jat_pyin_decode: workspace of %zu bytes, %zu needed", work_bytes, need);
  JCHK(upload(h));
  hipStream_t s = (hipStream_t)stream;
  KCHK(pyin_forward_launch(h->plan, log_obs, B, frames, (uint16_t*)work, state, s));
  KCHK(pyin_trace_launch(h->plan, B, frames, (const uint16_t*)work, state, f0, voiced, s));
  return JAT_OK;
}

int jat_pyin_set_profile(jat_pyin* h, int32_t on) {
  if (!h) return fail(JAT_E_INVALID, "jat_pyin_set_profile: null handle");
  h->profile = on != 0;
  return JAT_OK;
}

int jat_pyin_profile(jat_pyin* h, float* us) {
  if (!h || !us) return fail(JAT_E_INVALID, "jat_pyin_profile: null pointer");
  if (!h->profile || !h->ev[4]) return fail(JAT_E_STATE, "jat_pyin_profile: no profiled jat_pyin_track has run");
  HIPCHK(hipEventSynchronize(h->ev[4]));
  for (int i = 0; i < 4; ++i) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, h->ev[i], h->ev[i + 1]));
    us[i] = ms * 1e3f;
  }
  return JAT_OK;
}

}  // extern "C"
