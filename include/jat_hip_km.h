/*
 * jat_hip_km.h — C ABI of k-means compaction of a retrieval bank, an addition to jat_hip.h: a large pool of
 * latent frames is clustered on the GPU and its K centroids become an ordinary bank, the way RVC's index training stores
 * k-means centroids instead of every feature.  The conventions of jat_hip.h hold: device pointers unless marked [host], every
 * call only enqueues on the caller's stream, none of them synchronises, allocates or copies between host and device, and each
 * may be captured into a graph.
 *
 * Definitions
 *   Pool and centroids.  The pool is a jat_bank of 1 <= N <= JAT_KM_MAX_POOL = 2^22 normalised fp16 rows, filled by
 *     jat_bank_add / jat_bank_add_pooled / jat_bank_load_rows.  The centroids are a second jat_bank of the same channel count
 *     and the same pairedness holding K rows, 1 <= K <= N.  Banks of mixed pairedness or channel count: JAT_E_INVALID.
 *   Assignment.  For pool row n and centroid i < K
 *         d(n, i) = (|q_n|^2 + |k_i|^2) - 2 q_n.k_i
 *     with the two fp32 norms the banks store and the product exact in both fp16 operands, accumulated in fp32 over ascending
 *     16-channel steps (v_mfma_f32_32x32x16_f16, ONE pass: pool rows are fp16 already, so the hi / lo split that
 *     jat_bank_search needs for fp32 queries has nothing to split).  idx[n] = argmin_i d(n, i), the lowest i on equal d;
 *     dist2[n] = max(d, 0).  The result for a row depends on the row and the centroids alone: not on first / count, the grid,
 *     the row's place in its tile or the run.  The pool is read row-major as it is stored.
 *   Update.  Every finite fp16 value is an integer multiple of 2^-24 of magnitude below 2^40 in those units, so for cluster i
 *     with member set M_i (n_i members) the per-channel sum S = sum_{n in M_i} row[n, c] 2^24 is an exact int64
 *     (2^22 2^40 = 2^62: hence N <= 2^22).  The new row is
 *         fp16_rne( fp32_rne( double_rne(S) / double(n_i) ) 2^-24 ),
 *     for the keys, and for the values of a paired bank; the norms are recomputed by the kernel every bank entry uses.  A cluster
 *     with n_i = 0 keeps its row and its norm bit for bit.  counts[i] = n_i.  S is exact, so the order in which members are
 *     visited (it varies from run to run) does not reach the result.  Rows that are not finite are outside this contract.
 *   Inertia.  sum_n dist2[n] in fp64 in one fixed order: the same bits on every run.
 */
#ifndef JAT_HIP_KM_H
#define JAT_HIP_KM_H

#include "jat_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define JAT_KM_MAX_POOL 4194304   /* 2^22 pool rows at most: the int64 channel sums stay exact */

/* Bytes of workspace jat_bank_assign needs for `count` pool rows.  The assignment scans every centroid inside one workgroup
 * and keeps no partials: this is a small constant, kept so that callers size and pass a buffer like for every other entry. */
int jat_bank_assign_workspace_bytes(const jat_bank* pool, const jat_bank* centroids, int64_t count, size_t* bytes);

/* idx int32 [count], dist2 fp32 [count] (may be NULL): the nearest centroid of pool rows first .. first + count - 1, as defined
 * above.  changed (may be NULL): one int32 that is INCREMENTED by the number of rows whose idx differs from the value the idx
 * buffer held on entry (the caller zeroes it; idx is therefore read before it is written and must be initialised, e.g. to -1).
 * JAT_E_INVALID: a range outside the pool, N > 2^22, K > N, mixed banks, too small a workspace; JAT_E_STATE: an empty bank. */
int jat_bank_assign(const jat_bank* pool, int64_t first, int64_t count, const jat_bank* centroids, int32_t* idx, float* dist2,
                    int32_t* changed, void* work, size_t work_bytes, void* stream);

/* Bytes of workspace jat_bank_cluster_update needs for this pool and K clusters (member lists and their offsets). */
int jat_bank_cluster_update_workspace_bytes(const jat_bank* pool, int32_t K, size_t* bytes);

/* Moves every centroid to the mean of its members as defined above.  idx int32 [N] over the WHOLE pool, counts int32 [K] (out).
 * An idx entry outside [0, K) cannot be reported without waiting for the device, so it is checked ON the device and the row is
 * skipped: it joins no cluster and is never used as an address; sum(counts) < N is how a caller sees it (the Python wrapper of
 * jatsr_amd.retrieval checks exactly that and raises).  JAT_E_INVALID: K is not the centroid bank's size, K > N, N > 2^22,
 * mixed banks, too small a workspace. */
int jat_bank_cluster_update(const jat_bank* pool, const int32_t* idx, jat_bank* centroids, int32_t* counts, void* work,
                            size_t work_bytes, void* stream);

/* out[0] (one device double) = dist2[0] + ... + dist2[n - 1] in fp64, one fixed order (1024 strided partial sums, ascending,
 * then a fixed tree).  1 <= n <= 2^31 - 1. */
int jat_bank_sum_dist2(const float* dist2, int64_t n, double* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* JAT_HIP_KM_H */
