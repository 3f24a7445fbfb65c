// C ABI of k-means compaction (include/jat_hip_km.h): the argument checks and the launches of retrieval_km.hip.  Nothing here
// allocates, synchronises or copies: the workspaces come from the caller.
#include "jat_internal.h"
#include "jat_retrieval_km_kernels.h"
#include "jat_bank.h"
#include "../../include/jat_hip_km.h"

namespace {

static_assert(JAT_KM_MAX_POOL == KM_MAX_POOL, "header and kernel disagree");
constexpr size_t kAssignBytes = 256;   // the assignment keeps no partials; a token buffer keeps the call's shape

// pool and centroids as a pair: two different banks of one channel count and one pairedness, N <= 2^22
int check_pair(const char* who, const jat_bank* pool, const jat_bank* cent) {
  if (!pool || !cent) return fail(JAT_E_INVALID, "%s: null bank", who);
  if (pool == cent) return fail(JAT_E_INVALID, "%s: the pool and the centroids are the same bank", who);
  if (pool->channels != cent->channels)
    return fail(JAT_E_INVALID, "%s: pool of %d channels, centroids of %d", who, pool->channels, cent->channels);
  if (pool->paired != cent->paired)
    return fail(JAT_E_INVALID, "%s: the pool is %spaired, the centroids are %spaired", who, pool->paired ? "" : "not ",
                cent->paired ? "" : "not ");
  return JAT_OK;
}

int check_sizes(const char* who, int64_t N, int64_t K) {
  if (N < 1 || K < 1) return fail(JAT_E_STATE, "%s: an empty bank (pool %lld rows, centroids %lld)", who, (long long)N, (long long)K);
  if (N > KM_MAX_POOL) return fail(JAT_E_INVALID, "%s: pool of %lld rows exceeds 2^22", who, (long long)N);
  if (K > N) return fail(JAT_E_INVALID, "%s: %lld centroids for a pool of %lld rows", who, (long long)K, (long long)N);
  return JAT_OK;
}

size_t update_part(size_t n) { return align_up(n * sizeof(int32_t), 256); }
size_t update_bytes(int64_t N, int64_t K) { return 2 * update_part((size_t)K) + update_part((size_t)N); }

}  // namespace

extern "C" {

int jat_bank_assign_workspace_bytes(const jat_bank* pool, const jat_bank* centroids, int64_t count, size_t* bytes) {
  JCHK(check_pair("jat_bank_assign_workspace_bytes", pool, centroids));
  if (!bytes) return fail(JAT_E_INVALID, "jat_bank_assign_workspace_bytes: null output pointer");
  if (count < 1 || count > KM_MAX_POOL)
    return fail(JAT_E_INVALID, "jat_bank_assign_workspace_bytes: %lld rows outside 1..2^22", (long long)count);
  *bytes = kAssignBytes;
  return JAT_OK;
}

int jat_bank_assign(const jat_bank* pool, int64_t first, int64_t count, const jat_bank* centroids, int32_t* idx, float* dist2,
                    int32_t* changed, void* work, size_t work_bytes, void* stream) {
  JCHK(check_pair("jat_bank_assign", pool, centroids));
  JCHK(check_sizes("jat_bank_assign", pool->size, centroids->size));
  if (!idx || !work) return fail(JAT_E_INVALID, "jat_bank_assign: null buffer");
  if (work_bytes < kAssignBytes) return fail(JAT_E_INVALID, "jat_bank_assign: workspace %zu < %zu bytes", work_bytes, kAssignBytes);
  if (first < 0 || count < 1 || first >= pool->size || count > pool->size - first)
    return fail(JAT_E_INVALID, "jat_bank_assign: rows %lld .. +%lld leave the %d rows of the pool", (long long)first,
                (long long)count, pool->size);
  KCHK(km_assign_launch(pool->keys, pool->norms, first, (int)count, centroids->keys, centroids->norms, centroids->size,
                        pool->channels, idx, dist2, changed, (hipStream_t)stream));
  return JAT_OK;
}

int jat_bank_cluster_update_workspace_bytes(const jat_bank* pool, int32_t K, size_t* bytes) {
  if (!pool) return fail(JAT_E_INVALID, "jat_bank_cluster_update_workspace_bytes: null bank");
  if (!bytes) return fail(JAT_E_INVALID, "jat_bank_cluster_update_workspace_bytes: null output pointer");
  if (K < 1) return fail(JAT_E_INVALID, "jat_bank_cluster_update_workspace_bytes: K %d must be at least 1", K);
  JCHK(check_sizes("jat_bank_cluster_update_workspace_bytes", pool->size, K));
  *bytes = update_bytes(pool->size, K);
  return JAT_OK;
}

int jat_bank_cluster_update(const jat_bank* pool, const int32_t* idx, jat_bank* centroids, int32_t* counts, void* work,
                            size_t work_bytes, void* stream) {
  JCHK(check_pair("jat_bank_cluster_update", pool, centroids));
  const int N = pool->size, K = centroids->size;
  JCHK(check_sizes("jat_bank_cluster_update", N, K));
  if (!idx || !counts || !work) return fail(JAT_E_INVALID, "jat_bank_cluster_update: null buffer");
  if ((uintptr_t)work & 3) return fail(JAT_E_INVALID, "jat_bank_cluster_update: the workspace must be 4-byte aligned");
  const size_t need = update_bytes(N, K);
  if (work_bytes < need) return fail(JAT_E_INVALID, "jat_bank_cluster_update: workspace %zu < %zu bytes", work_bytes, need);
  hipStream_t s = (hipStream_t)stream;
  int32_t* offsets = (int32_t*)work;
  int32_t* cursor = (int32_t*)((char*)work + update_part((size_t)K));
  int32_t* members = (int32_t*)((char*)work + 2 * update_part((size_t)K));
  KCHK(km_update_launch(pool->keys, pool->paired ? pool->values : nullptr, idx, N, centroids->keys,
                        centroids->paired ? centroids->values : nullptr, K, pool->channels, counts, offsets, cursor, members, s));
  KCHK(bank_norms_launch(centroids->keys, centroids->norms, 0, K, centroids->channels, s));
  return JAT_OK;
}

int jat_bank_sum_dist2(const float* dist2, int64_t n, double* out, void* stream) {
  if (!dist2 || !out) return fail(JAT_E_INVALID, "jat_bank_sum_dist2: null buffer");
  if (n < 1 || n > 0x7fffffffLL) return fail(JAT_E_INVALID, "jat_bank_sum_dist2: %lld values outside 1..2^31-1", (long long)n);
  KCHK(km_sum_dist2_launch(dist2, n, out, (hipStream_t)stream));
  return JAT_OK;
}

}  // extern "C"
