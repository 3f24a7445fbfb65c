/*
 * jat_hip_ivf.h — C ABI of the IVF index over a retrieval bank, an addition to jat_hip.h and jat_hip_km.h: the
 * rows of a bank are grouped by their nearest centroid ("list"), and a search visits only the lists whose centroids are
 * nearest to the query, the way RVC's IVF{n},Flat index is searched with nprobe = 1.  The conventions of jat_hip.h hold:
 * device pointers unless marked [host], every call only enqueues on the caller's stream, none of them synchronises, allocates
 * or copies between host and device, and each may be captured into a graph.
 *
 * Definitions
 *   Index.  (a) a jat_bank whose rows are permuted so that the members of list 0 come first, then list 1, ...; inside a list
 *     the rows ascend by their original row number.  It is an ordinary bank: every entry of jat_hip.h works on it.
 *     (b) a centroid bank of nlist rows (only its keys and norms are read).  (c) offsets int32 [nlist + 1]: list l is the
 *     positions offsets[l] .. offsets[l + 1] - 1.  (d) order int32 [N]: the original row of every position (provenance).
 *     Every index the search returns is a POSITION in the permuted bank.
 *   Grouping.  idx int32 [N] as jat_bank_assign writes it.  order is the stable sort of the rows by idx: the same bits on every
 *     run.  An idx entry outside [0, nlist) is checked on the device and never used as an address; such rows are placed behind
 *     all lists, ascending by source row, belong to no list and are never returned by the search: offsets[nlist] < N is how a
 *     caller sees them.  dst keys, values and norms at position p are those of src row order[p], bit for bit.
 *     The order inside a list is found by ranking (a member's place is the number of smaller members of its list), which is
 *     quadratic in the length of a list: fine for the lists k-means makes, slow for a bank that is one list.
 *   Search.  Stage 1: the probed lists of query n are the first nprobe entries of jat_bank_search_topk(centroids, .., k = nprobe)
 *     (that entry point is called); an entry of -1 (nlist < nprobe) probes nothing.  Stage 2: over the rows p of the probed
 *     lists ordered by (d(q, p), p) the first k, with d(q, p) = (|q|^2 + |k_p|^2) - 2 q.k_p computed by the arithmetic chain of
 *     jat_bank_search: the query normalised and split hi = fp16(q), lo = fp16(q - hi); |q|^2 as eight phase sums (fmaf chains
 *     over channels cg, cg + 8, ..) added in ascending phase order; the product as v_mfma_f32_32x32x16_f16 over ascending
 *     16-channel steps, hi before lo, into one fp32 accumulator.  dist2 = max(d, 0); places beyond the number of candidates
 *     hold idx -1 and dist2 +inf.  The result for a query is jat_bank_search_topk restricted to the probed lists, bit for bit;
 *     with nprobe >= nlist it is jat_bank_search_topk on the permuted bank.  It depends on the query, the bank, the centroids
 *     and the offsets alone: not on B, on neighbouring queries, on the grid or on the run.
 */
#ifndef JAT_HIP_IVF_H
#define JAT_HIP_IVF_H

#include "jat_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define JAT_IVF_MAX_NPROBE 8
#define JAT_IVF_MAX_ROWS 4194304   /* 2^22 rows at most: the limit of jat_bank_assign */

/* Bytes of workspace jat_bank_group needs for this bank and nlist lists (a cursor per list and the unsorted member lists). */
int jat_bank_group_workspace_bytes(const jat_bank* src, int32_t nlist, size_t* bytes);

/* Groups src by idx into dst as defined above.  dst: another bank of the same channel count and pairedness, capacity >= N,
 * EMPTY on entry; it ends with size N.  offsets int32 [nlist + 1] and order int32 [N] are outputs.  work: 4-byte aligned.
 * JAT_E_INVALID: mixed banks, src == dst, nlist outside 1..N, N > 2^22, dst too small, too small a workspace;
 * JAT_E_STATE: an empty src or a dst that is not empty. */
int jat_bank_group(const jat_bank* src, const int32_t* idx, int32_t nlist, jat_bank* dst, int32_t* offsets, int32_t* order,
                   void* work, size_t work_bytes, void* stream);

/* Bytes of workspace jat_ivf_search needs: the workspace of the coarse jat_bank_search_topk, the probed lists, and the
 * normalised query planes (two fp16 planes and |q|^2 per query). */
int jat_ivf_search_workspace_bytes(const jat_bank* bank, const jat_bank* centroids, int64_t n_queries, int32_t k,
                                   int32_t nprobe, size_t* bytes);

/* x fp32 [B, C, T], mean / std fp32 [C] (both or neither), as in jat_bank_search.  offsets int32 [centroids' size + 1]: a list
 * that leaves [0, bank's size] is clipped to it on the device.  idx int32 [B T, k]; dist2 fp32 [B T, k] (may be NULL);
 * probes int32 [B T, nprobe] (may be NULL): the probed lists.  work: 8-byte aligned.
 * JAT_E_INVALID: k outside 1..JAT_BANK_MAX_K, nprobe outside 1..JAT_IVF_MAX_NPROBE, mixed channel counts, bank == centroids,
 * a bank above 2^22 rows, a null buffer, too small a workspace; JAT_E_STATE: an empty bank or no centroids. */
int jat_ivf_search(jat_bank* bank, jat_bank* centroids, const int32_t* offsets, const float* x, const float* mean,
                   const float* std, int32_t B, int32_t T, int32_t k, int32_t nprobe, int32_t* idx, float* dist2,
                   int32_t* probes, void* work, size_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* JAT_HIP_IVF_H */
