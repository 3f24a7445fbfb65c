// C ABI of the IIR low-pass cascades (include/jat_hip_iir.h): the filter table (fp64 on the host -> fp32 on the device), the
// argument checks, the workspace layout and the launches of iir.hip.  The filtering calls allocate, copy and wait for nothing.
#include <algorithm>
#include <cmath>
#include <vector>

#include "jat_internal.h"
#include "jat_iir_kernels.h"
#include "../../include/jat_hip_iir.h"

struct jat_iir {
  int R = 0, padlen = 0;          // padlen: the largest of the table
  IirFilter* tab = nullptr;       // device [R]
};

namespace {

static_assert(JAT_IIR_SECTIONS == IIR_SECTIONS && JAT_IIR_POWERS == IIR_POWERS && JAT_IIR_MAX_PADLEN == IIR_MAX_PADLEN,
              "header and kernel disagree");

bool identity(const double* s) { return s[0] == 1.0 && s[1] == 0.0 && s[2] == 0.0 && s[4] == 0.0 && s[5] == 0.0; }

// [ext | states]: the filtered extension of sosfiltfilt's forward pass, then the tile states
size_t ext_bytes(int32_t B, int64_t n) { return align_up((size_t)B * ((size_t)n + 2 * IIR_MAX_PADLEN) * sizeof(float), 256); }
size_t state_bytes(int32_t B, int64_t n) { return (size_t)B * iir_tiles(n) * IIR_STATE * sizeof(float); }

int check_call(const char* who, const jat_iir* h, const int32_t* row_filter, const float* x, const float* y, int32_t B, int64_t n,
               const void* work, size_t work_bytes) {
  if (!h) return fail(JAT_E_INVALID, "%s: null handle", who);
  if (B < 1 || B > 65535) return fail(JAT_E_INVALID, "%s: batch %d outside 1..65535", who, B);
  if (n < 1 || n > JAT_IIR_MAX_N) return fail(JAT_E_INVALID, "%s: length %lld outside 1..%d", who, (long long)n, JAT_IIR_MAX_N);
  if (!row_filter || !x || !y || !work) return fail(JAT_E_INVALID, "%s: null buffer", who);
  const size_t need = ext_bytes(B, n) + state_bytes(B, n);
  if (work_bytes < need) return fail(JAT_E_STATE, "%s: workspace %zu < %zu bytes", who, work_bytes, need);
  return JAT_OK;
}

}  // namespace

extern "C" {

int jat_iir_create(const double* sos, const double* zi, const double* powers, int32_t R, void* stream, void** handle) {
  if (!handle) return fail(JAT_E_INVALID, "jat_iir_create: null output pointer");
  *handle = nullptr;
  if (!sos || !zi || !powers) return fail(JAT_E_INVALID, "jat_iir_create: null table");
  if (R < 1 || R > JAT_IIR_MAX_FILTERS) return fail(JAT_E_INVALID, "jat_iir_create: %d filters outside 1..%d", R, JAT_IIR_MAX_FILTERS);
  std::vector<IirFilter> tab((size_t)R);
  int padlen = 0;
  for (int r = 0; r < R; ++r) {
    IirFilter& F = tab[r];
    const double* s = sos + (size_t)r * IIR_SECTIONS * 6;
    int nsec = 0, b2z = 0, a2z = 0;
    for (int k = 0; k < IIR_SECTIONS; ++k) {
      for (int c = 0; c < 6; ++c)
        if (!std::isfinite(s[k * 6 + c])) return fail(JAT_E_INVALID, "jat_iir_create: filter %d section %d is not finite", r, k);
      if (s[k * 6 + 3] != 1.0) return fail(JAT_E_INVALID, "jat_iir_create: filter %d section %d has a0 = %g, must be 1", r, k, s[k * 6 + 3]);
      if (!identity(s + k * 6)) nsec = k + 1;
      const double* q = s + k * 6;
      const float c5[5] = {(float)q[0], (float)q[1], (float)q[2], (float)q[4], (float)q[5]};
      for (int c = 0; c < 5; ++c) F.c[k][c] = c5[c];
    }
    for (int k = 0; k < nsec; ++k) {
      if (identity(s + k * 6))
        return fail(JAT_E_INVALID, "jat_iir_create: filter %d has an identity section in front of section %d", r, nsec - 1);
      b2z += s[k * 6 + 2] == 0.0;
      a2z += s[k * 6 + 5] == 0.0;
    }
    F.nsec = nsec;
    F.padlen = 3 * (2 * nsec + 1 - std::min(b2z, a2z));
    F.pad[0] = F.pad[1] = F.pad[2] = 0;
    padlen = std::max(padlen, F.padlen);
    for (int c = 0; c < IIR_STATE; ++c) {
      const double v = zi[(size_t)r * IIR_STATE + c];
      if (!std::isfinite(v)) return fail(JAT_E_INVALID, "jat_iir_create: filter %d has a zi that is not finite", r);
      F.zi[c] = (float)v;
    }
    const double* pw = powers + (size_t)r * IIR_POWERS * IIR_STATE * IIR_STATE;
    for (int c = 0; c < IIR_POWERS * IIR_STATE * IIR_STATE; ++c) {
      if (!std::isfinite(pw[c])) return fail(JAT_E_INVALID, "jat_iir_create: filter %d has a power matrix that is not finite", r);
      F.pw[0][c] = (float)pw[c];
    }
  }
  std::unique_ptr<jat_iir> h(new jat_iir);
  h->R = R, h->padlen = padlen;
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipMalloc(&h->tab, tab.size() * sizeof(IirFilter)));
  hipError_t e = hipMemcpyAsync(h->tab, tab.data(), tab.size() * sizeof(IirFilter), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);   // tab leaves scope
  if (e != hipSuccess) {
    (void)hipFree(h->tab);
    return fail(JAT_E_HIP, "jat_iir_create: table upload failed: %s", hipGetErrorString(e));
  }
  *handle = h.release();
  return JAT_OK;
}

void jat_iir_destroy(void* handle) {
  jat_iir* h = (jat_iir*)handle;
  if (!h) return;
  if (h->tab) (void)hipFree(h->tab);
  delete h;
}

int jat_iir_geometry(int32_t* lane_block, int32_t* tile) {
  if (lane_block) *lane_block = IIR_LANE_BLOCK;
  if (tile) *tile = IIR_TILE;
  return JAT_OK;
}

int jat_iir_padlen(const void* handle, int32_t* padlen) {
  if (!handle || !padlen) return fail(JAT_E_INVALID, "jat_iir_padlen: null argument");
  *padlen = ((const jat_iir*)handle)->padlen;
  return JAT_OK;
}

int jat_iir_workspace_bytes(int32_t B, int64_t n, size_t* bytes) {
  if (!bytes) return fail(JAT_E_INVALID, "jat_iir_workspace_bytes: null output pointer");
  if (B < 1 || B > 65535) return fail(JAT_E_INVALID, "jat_iir_workspace_bytes: batch %d outside 1..65535", B);
  if (n < 1 || n > JAT_IIR_MAX_N)
    return fail(JAT_E_INVALID, "jat_iir_workspace_bytes: length %lld outside 1..%d", (long long)n, JAT_IIR_MAX_N);
  *bytes = ext_bytes(B, n) + state_bytes(B, n);
  return JAT_OK;
}

int jat_iir_sosfilt(void* handle, const int32_t* row_filter, const float* x, float* y, int32_t B, int64_t n, void* workspace,
                    size_t workspace_bytes, void* stream) {
  const jat_iir* h = (const jat_iir*)handle;
  JCHK(check_call("jat_iir_sosfilt", h, row_filter, x, y, B, n, workspace, workspace_bytes));
  float* states = (float*)((char*)workspace + ext_bytes(B, n));
  KCHK(iir_pass_launch(h->tab, h->R, row_filter, x, y, states, B, (int)n, IIR_PLAIN, (hipStream_t)stream));
  return JAT_OK;
}

int jat_iir_sosfiltfilt(void* handle, const int32_t* row_filter, const float* x, float* y, int32_t B, int64_t n, void* workspace,
                        size_t workspace_bytes, void* stream) {
  const jat_iir* h = (const jat_iir*)handle;
  JCHK(check_call("jat_iir_sosfiltfilt", h, row_filter, x, y, B, n, workspace, workspace_bytes));
  if (n <= h->padlen)
    return fail(JAT_E_INVALID, "jat_iir_sosfiltfilt: length %lld must be greater than padlen %d", (long long)n, h->padlen);
  float* ext = (float*)workspace;
  float* states = (float*)((char*)workspace + ext_bytes(B, n));
  hipStream_t s = (hipStream_t)stream;
  KCHK(iir_pass_launch(h->tab, h->R, row_filter, x, ext, states, B, (int)n, IIR_FORWARD, s));
  KCHK(iir_pass_launch(h->tab, h->R, row_filter, ext, y, states, B, (int)n, IIR_BACKWARD, s));
  return JAT_OK;
}

}  // extern "C"
