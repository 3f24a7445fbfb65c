// C ABI of the sample-rate converter and the per-channel latent statistics (include/jat_hip.h): the tap table in fp64 on
// the host, the resampler handle, the launches of resample.hip.
#include <cmath>
#include <numeric>
#include <vector>

#include "jat_internal.h"
#include "jat_resample_kernels.h"

struct jat_resampler {
  int orig = 0, new_ = 0, lpw = 0, o = 0, n = 0, width = 0, K = 0;
  double rolloff = 0.0;
  float* table = nullptr;   // device, transposed [K][n]; null for orig == new (a copy)
  ResampleGeom geom;
};

namespace {

static_assert(STATS_SLICES == JAT_STATS_SLICES, "resample.hip and jat_hip.h disagree");
constexpr int64_t kMaxTable = (int64_t)1 << 26;   // tap-table entries (256 MiB): coprime rates ask for far more
constexpr int64_t kMax31 = 0x7fffffff;

int table_dims(int orig, int new_, int lpw, double rolloff, int* o, int* n, int* width, int* K) {
  if (orig < 1 || new_ < 1) return fail(JAT_E_INVALID, "resample: sample rates %d -> %d must be positive", orig, new_);
  if (lpw < 1) return fail(JAT_E_INVALID, "resample: lowpass_filter_width %d must be >= 1", lpw);
  if (!(rolloff > 0.0 && rolloff <= 1.0)) return fail(JAT_E_INVALID, "resample: rolloff %g outside (0, 1]", rolloff);
  const int g = std::gcd(orig, new_);
  *o = orig / g;
  *n = new_ / g;
  const double base = std::min(*o, *n) * rolloff;
  const double w = std::ceil((double)lpw * *o / base);
  if (w > (double)(1 << 24)) return fail(JAT_E_INVALID, "resample: %d -> %d needs a filter of %g taps a side", orig, new_, w);
  *width = (int)w;
  *K = 2 * *width + *o;
  if ((int64_t)*n * *K > kMaxTable)
    return fail(JAT_E_INVALID, "resample: %d -> %d needs a table of %d x %d taps (limit %lld entries)", orig, new_, *n, *K,
                (long long)kMaxTable);
  return JAT_OK;
}

// h[p][k] of torchaudio's _get_sinc_resample_kernel (sinc_interp_hann), every step in fp64
double tap(int p, int k, int o, int n, int width, int lpw, double base) {
  const double pi = 3.14159265358979323846;
  double t = (-(double)p / n + (double)(k - width) / o) * base;
  t = std::min(std::max(t, -(double)lpw), (double)lpw);
  const double c = std::cos(t * pi / lpw / 2.0);
  const double s = t == 0.0 ? 1.0 : std::sin(pi * t) / (pi * t);
  return s * (c * c) * (base / o);
}

// the checks of jat_resampler_create that need no GPU: the table's dimensions, then a block shape whose window fits
int plan_dims(int orig, int new_, int lpw, double rolloff, int* o, int* n, int* width, int* K, ResampleGeom* geom) {
  JCHK(table_dims(orig, new_, lpw, rolloff, o, n, width, K));
  if (*o != *n && !resample_geometry(*o, *n, *K, geom))
    return fail(JAT_E_INVALID, "resample: %d -> %d: a window of %d + 7 x %d samples does not fit one block (limit %d)", orig,
                new_, *K, *o, RS_MAX_WINDOW);
  return JAT_OK;
}

// L_out = ceil(n L / o), refused as include/jat_hip.h says
int out_length(int orig, int new_, int o, int n, int K, int64_t L, int64_t* L_out) {
  if (L < 0) return fail(JAT_E_INVALID, "resample: length %lld is negative", (long long)L);
  if (L + K > kMax31 || L > (kMax31 - o) / n * o)   // the second bound keeps ceil(n L / o) within 31 bits
    return fail(JAT_E_INVALID, "resample: length %lld (%d -> %d) does not fit 31 bits", (long long)L, orig, new_);
  *L_out = (L * n + o - 1) / o;
  return JAT_OK;
}

}  // namespace

extern "C" {

int jat_resample_table(int32_t orig, int32_t new_, int32_t lpw, double rolloff, float* table, int32_t* o, int32_t* n,
                       int32_t* width, int32_t* K) {
  if (!o || !n || !width || !K) return fail(JAT_E_INVALID, "jat_resample_table: null output pointer");
  int o_, n_, w_, k_;
  JCHK(table_dims(orig, new_, lpw, rolloff, &o_, &n_, &w_, &k_));
  *o = o_, *n = n_, *width = w_, *K = k_;
  if (table) {
    const double base = std::min(o_, n_) * rolloff;
    for (int p = 0; p < n_; ++p)
      for (int k = 0; k < k_; ++k) table[(size_t)p * k_ + k] = (float)tap(p, k, o_, n_, w_, lpw, base);
  }
  return JAT_OK;
}

int jat_resampler_create(int32_t orig, int32_t new_, int32_t lpw, double rolloff, void* stream, jat_resampler** out) {
  if (!out) return fail(JAT_E_INVALID, "jat_resampler_create: null output pointer");
  *out = nullptr;
  std::unique_ptr<jat_resampler> r(new jat_resampler);
  r->orig = orig, r->new_ = new_, r->lpw = lpw, r->rolloff = rolloff;
  JCHK(plan_dims(orig, new_, lpw, rolloff, &r->o, &r->n, &r->width, &r->K, &r->geom));
  if (r->o != r->n) {
    const double base = std::min(r->o, r->n) * rolloff;
    std::vector<float> ht((size_t)r->K * r->n);
    for (int p = 0; p < r->n; ++p)
      for (int k = 0; k < r->K; ++k) ht[(size_t)k * r->n + p] = (float)tap(p, k, r->o, r->n, r->width, lpw, base);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMalloc(&r->table, ht.size() * sizeof(float)));
    hipError_t e = hipMemcpyAsync(r->table, ht.data(), ht.size() * sizeof(float), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);   // ht leaves scope
    if (e != hipSuccess) {
      (void)hipFree(r->table);
      return fail(JAT_E_HIP, "jat_resampler_create: table upload failed: %s", hipGetErrorString(e));
    }
  }
  *out = r.release();
  return JAT_OK;
}

void jat_resampler_destroy(jat_resampler* r) {
  if (!r) return;
  if (r->table) (void)hipFree(r->table);
  delete r;
}

int jat_resample_out_length(const jat_resampler* r, int64_t L, int64_t* L_out) {
  if (!r || !L_out) return fail(JAT_E_INVALID, "jat_resample_out_length: null argument");
  return out_length(r->orig, r->new_, r->o, r->n, r->K, L, L_out);
}

int jat_k_resample_geometry(int32_t orig, int32_t new_, int32_t lpw, double rolloff, int64_t L, int32_t* K, int32_t* ph,
                            int32_t* pn, int32_t* slices, int32_t* lanes, int32_t* groups_max, int32_t* groups,
                            int32_t* grid_x, int32_t* block, int32_t* lds_bytes) {
  int o, n, width, k;
  ResampleGeom g;
  JCHK(plan_dims(orig, new_, lpw, rolloff, &o, &n, &width, &k, &g));
  int64_t L_out = 0;
  JCHK(out_length(orig, new_, o, n, k, L, &L_out));
  ResampleLaunch a;                                   // all zero: orig == new is a copy and L == 0 launches nothing
  if (o == n) g = ResampleGeom{0, 0, 0, 0, 0};
  else if (L > 0) a = resample_launch_shape(g, (int)L_out, o, n, k);
  const int32_t vals[10] = {k, g.ph, g.pn, g.slices, g.lanes, g.groups, a.groups, (int32_t)a.grid_x, a.block, (int32_t)a.lds};
  int32_t* const outs[10] = {K, ph, pn, slices, lanes, groups_max, groups, grid_x, block, lds_bytes};
  for (int i = 0; i < 10; ++i)
    if (outs[i]) *outs[i] = vals[i];
  return JAT_OK;
}

int jat_resample(jat_resampler* r, const float* x, float* y, int32_t B, int64_t L, void* stream) {
  if (!r) return fail(JAT_E_INVALID, "jat_resample: null handle");
  if (B < 1 || B > 65535) return fail(JAT_E_INVALID, "resample: batch %d outside 1..65535", B);
  int64_t L_out = 0;
  JCHK(jat_resample_out_length(r, L, &L_out));
  if (L == 0) return JAT_OK;
  if (!x || !y) return fail(JAT_E_INVALID, "jat_resample: null buffer");
  hipStream_t s = (hipStream_t)stream;
  if (r->o == r->n) {
    if (x != y) HIPCHK(hipMemcpyAsync(y, x, (size_t)B * L * sizeof(float), hipMemcpyDeviceToDevice, s));
    return JAT_OK;
  }
  KCHK(resample_launch(x, y, r->table, B, (int)L, (int)L_out, r->o, r->n, r->width, r->K, r->geom, s));
  return JAT_OK;
}

int jat_channel_stats(const float* z, int32_t B, int32_t C, int32_t T, double* sum, double* sq_sum, void* work,
                      size_t work_bytes, void* stream) {
  if (!z || !sum || !sq_sum || !work) return fail(JAT_E_INVALID, "jat_channel_stats: null buffer");
  if (B < 1 || C < 1 || T < 1) return fail(JAT_E_INVALID, "jat_channel_stats: shape [%d, %d, %d]", B, C, T);
  if (C > 65535) return fail(JAT_E_INVALID, "jat_channel_stats: %d channels (limit 65535)", C);
  const size_t need = (size_t)C * JAT_STATS_SLICES * 2 * sizeof(double);
  if (work_bytes < need) return fail(JAT_E_STATE, "jat_channel_stats: workspace %zu < %zu bytes", work_bytes, need);
  KCHK(channel_stats_launch(z, B, C, T, (double*)work, sum, sq_sum, (hipStream_t)stream));
  return JAT_OK;
}

}  // extern "C"
