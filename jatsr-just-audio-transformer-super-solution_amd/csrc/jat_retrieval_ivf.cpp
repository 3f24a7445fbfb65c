// C ABI of the IVF index (include/jat_hip_ivf.h): the argument checks and the launches of retrieval_ivf.hip.  Nothing here
// allocates, synchronises or copies: the workspaces come from the caller.  The coarse stage is jat_bank_search_topk itself.
#include "jat_internal.h"
#include "jat_retrieval_ivf_kernels.h"
#include "jat_bank.h"
#include "../../include/jat_hip_ivf.h"

namespace {

static_assert(JAT_IVF_MAX_NPROBE == IVF_MAX_NPROBE && JAT_IVF_MAX_ROWS == IVF_MAX_ROWS && JAT_BANK_MAX_K == RT_MAX_K,
              "header and kernel disagree");
constexpr int64_t kMaxQueries = 0x7fffffff / 2;   // what jat_bank_search_topk takes

// two different banks of one channel count (the search reads the centroids' keys only: their pairedness is free)
int check_pair(const char* who, const jat_bank* a, const jat_bank* b, bool same_pairedness) {
  if (!a || !b) return fail(JAT_E_INVALID, "%s: null bank", who);
  if (a == b) return fail(JAT_E_INVALID, "%s: both banks are the same bank", who);
  if (a->channels != b->channels)
    return fail(JAT_E_INVALID, "%s: banks of %d and of %d channels", who, a->channels, b->channels);
  if (same_pairedness && a->paired != b->paired)
    return fail(JAT_E_INVALID, "%s: one bank is paired, the other is not", who);
  return JAT_OK;
}

size_t part(size_t n) { return align_up(n, 256); }
size_t group_bytes(int64_t N, int64_t nlist) {
  return part((size_t)(nlist + 1) * sizeof(int32_t)) + part((size_t)N * sizeof(int32_t));
}

int check_search_shape(const char* who, int32_t k, int32_t nprobe) {
  if (k < 1 || k > JAT_BANK_MAX_K) return fail(JAT_E_INVALID, "%s: k %d outside 1..%d", who, k, JAT_BANK_MAX_K);
  if (nprobe < 1 || nprobe > JAT_IVF_MAX_NPROBE)
    return fail(JAT_E_INVALID, "%s: nprobe %d outside 1..%d", who, nprobe, JAT_IVF_MAX_NPROBE);
  return JAT_OK;
}

// the parts of the search workspace in order: coarse top-k, probes, hi plane, lo plane, |q|^2
struct SearchParts { size_t coarse, probes, plane, qn, total; };
int search_parts(const jat_bank* centroids, int64_t nq, int32_t nprobe, SearchParts* p) {
  JCHK(jat_bank_topk_workspace_bytes(centroids, nq, nprobe, &p->coarse));
  p->coarse = part(p->coarse);
  p->probes = part((size_t)nq * nprobe * sizeof(int32_t));
  p->plane = part((size_t)nq * ivf_padded_channels(centroids->channels) * sizeof(uint16_t));
  p->qn = part((size_t)nq * sizeof(float));
  p->total = p->coarse + p->probes + 2 * p->plane + p->qn;
  return JAT_OK;
}

}  // namespace

extern "C" {

int jat_bank_group_workspace_bytes(const jat_bank* src, int32_t nlist, size_t* bytes) {
  if (!src) return fail(JAT_E_INVALID, "jat_bank_group_workspace_bytes: null bank");
  if (!bytes) return fail(JAT_E_INVALID, "jat_bank_group_workspace_bytes: null output pointer");
  if (src->size < 1) return fail(JAT_E_STATE, "jat_bank_group_workspace_bytes: the bank is empty");
  if (src->size > IVF_MAX_ROWS)
    return fail(JAT_E_INVALID, "jat_bank_group_workspace_bytes: bank of %d rows exceeds 2^22", src->size);
  if (nlist < 1 || nlist > src->size)
    return fail(JAT_E_INVALID, "jat_bank_group_workspace_bytes: %d lists for a bank of %d rows", nlist, src->size);
  *bytes = group_bytes(src->size, nlist);
  return JAT_OK;
}

int jat_bank_group(const jat_bank* src, const int32_t* idx, int32_t nlist, jat_bank* dst, int32_t* offsets, int32_t* order,
                   void* work, size_t work_bytes, void* stream) {
  JCHK(check_pair("jat_bank_group", src, dst, true));
  const int N = src->size;
  if (N < 1) return fail(JAT_E_STATE, "jat_bank_group: the source bank is empty");
  if (N > IVF_MAX_ROWS) return fail(JAT_E_INVALID, "jat_bank_group: bank of %d rows exceeds 2^22", N);
  if (nlist < 1 || nlist > N) return fail(JAT_E_INVALID, "jat_bank_group: %d lists for a bank of %d rows", nlist, N);
  if (dst->size != 0) return fail(JAT_E_STATE, "jat_bank_group: the destination holds %d rows, it must be empty", dst->size);
  if (dst->capacity < N) return fail(JAT_E_INVALID, "jat_bank_group: destination capacity %d < %d rows", dst->capacity, N);
  if (!idx || !offsets || !order || !work) return fail(JAT_E_INVALID, "jat_bank_group: null buffer");
  if ((uintptr_t)work & 3) return fail(JAT_E_INVALID, "jat_bank_group: the workspace must be 4-byte aligned");
  const size_t need = group_bytes(N, nlist);
  if (work_bytes < need) return fail(JAT_E_INVALID, "jat_bank_group: workspace %zu < %zu bytes", work_bytes, need);
  int32_t* cursor = (int32_t*)work;
  int32_t* members = (int32_t*)((char*)work + part((size_t)(nlist + 1) * sizeof(int32_t)));
  KCHK(ivf_group_launch(src->keys, src->paired ? src->values : nullptr, src->norms, idx, N, nlist, src->channels, dst->keys,
                        dst->paired ? dst->values : nullptr, dst->norms, offsets, order, cursor, members, (hipStream_t)stream));
  dst->size = N;
  return JAT_OK;
}

int jat_ivf_search_workspace_bytes(const jat_bank* bank, const jat_bank* centroids, int64_t n_queries, int32_t k,
                                   int32_t nprobe, size_t* bytes) {
  JCHK(check_pair("jat_ivf_search_workspace_bytes", bank, centroids, false));
  if (!bytes) return fail(JAT_E_INVALID, "jat_ivf_search_workspace_bytes: null output pointer");
  JCHK(check_search_shape("jat_ivf_search_workspace_bytes", k, nprobe));
  if (n_queries < 1 || n_queries > kMaxQueries)
    return fail(JAT_E_INVALID, "jat_ivf_search_workspace_bytes: %lld queries outside 1..2^30", (long long)n_queries);
  SearchParts p;
  JCHK(search_parts(centroids, n_queries, nprobe, &p));
  *bytes = p.total;
  return JAT_OK;
}

int jat_ivf_search(jat_bank* bank, jat_bank* centroids, const int32_t* offsets, const float* x, const float* mean,
                   const float* std, int32_t B, int32_t T, int32_t k, int32_t nprobe, int32_t* idx, float* dist2,
                   int32_t* probes, void* work, size_t work_bytes, void* stream) {
  JCHK(check_pair("jat_ivf_search", bank, centroids, false));
  JCHK(check_search_shape("jat_ivf_search", k, nprobe));
  if (B < 1 || B > 65535) return fail(JAT_E_INVALID, "jat_ivf_search: batch %d outside 1..65535", B);
  if (T < 1) return fail(JAT_E_INVALID, "jat_ivf_search: T %d must be at least 1", T);
  const int64_t nq = (int64_t)B * T;
  if (nq > kMaxQueries) return fail(JAT_E_INVALID, "jat_ivf_search: %d x %d queries do not fit 30 bits", B, T);
  if (!offsets || !x || !idx || !work) return fail(JAT_E_INVALID, "jat_ivf_search: null buffer");
  if ((mean != nullptr) != (std != nullptr)) return fail(JAT_E_INVALID, "jat_ivf_search: mean and std are both given or both null");
  if (bank->size > IVF_MAX_ROWS) return fail(JAT_E_INVALID, "jat_ivf_search: bank of %d rows exceeds 2^22", bank->size);
  if ((uintptr_t)work & 7) return fail(JAT_E_INVALID, "jat_ivf_search: the workspace must be 8-byte aligned");
  SearchParts p;
  JCHK(search_parts(centroids, nq, nprobe, &p));
  if (work_bytes < p.total) return fail(JAT_E_INVALID, "jat_ivf_search: workspace %zu < %zu bytes", work_bytes, p.total);
  if (bank->size < 1 || centroids->size < 1)
    return fail(JAT_E_STATE, "jat_ivf_search: an empty bank (%d rows, %d centroids)", bank->size, centroids->size);
  char* w = (char*)work;
  int32_t* pr = probes ? probes : (int32_t*)(w + p.coarse);
  uint16_t* qhi = (uint16_t*)(w + p.coarse + p.probes);
  uint16_t* qlo = (uint16_t*)(w + p.coarse + p.probes + p.plane);
  float* qn = (float*)(w + p.coarse + p.probes + 2 * p.plane);
  hipStream_t s = (hipStream_t)stream;
  // stage 1: the nprobe nearest centroids of every query, by the exact search itself
  JCHK(jat_bank_search_topk(centroids, x, mean, std, B, T, nprobe, pr, nullptr, w, p.coarse, stream));
  // stage 2: the probed lists
  KCHK(ivf_prepare_launch(x, mean, std, B, T, bank->channels, qhi, qlo, qn, s));
  KCHK(ivf_scan_launch(bank->keys, bank->norms, bank->size, bank->channels, offsets, centroids->size, pr, nprobe, qhi, qlo, qn,
                       nq, k, idx, dist2, s));
  return JAT_OK;
}

}  // extern "C"
