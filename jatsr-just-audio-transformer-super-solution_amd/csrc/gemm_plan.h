// Which tile variant (gemm_variants.h) and how many K slices each GEMM of the forward gets.  Host-only: no HIP calls.
#pragma once
#include "jat_internal.h"

// Small-M inference (the reference's own B = 1 chunk loop gives M = 690 rows with CFG; a file's short last chunk M = 240):
// the K = 5120 fc2 GEMM has a few dozen tiles x 80 K-steps — split K over otherwise idle CUs, finish in fixed order.
static constexpr int kSplitMaxRows = 2304, kSplitMax = 8;
static constexpr int kSplitWsRows = 4096;   // split-K partial workspace exists up to here (un-folded buckets: see plan_resid)
// slices the split-K partial workspace of a forward over M rows holds (0: it has none)
static inline int split_ws_slices(size_t M) { return M > (size_t)kSplitWsRows ? 0 : M <= (size_t)kSplitMaxRows ? kSplitMax : 2; }

struct GemmPlan { int variant, ksplit; };   // ksplit 1: no K slices

int pick_variant(int M, int N, int nbatch = 1);
// as many K slices as fill `slots` with `tiles` blocks each, at most `cap`; every slice whole 64-deep K-tiles and >= min_depth; 1 = none
int k_slices(long tiles, int slots, int cap, int K, int min_depth);

// One function per decision of the forward.  site: G_QKV ... G_OTHER; folding: a sampler bucket with folded norms; split_ws: the
// workspace has split-K partials (split_ws_slices(M) > 0).
// any GEMM [M, N] in `ksplit` slices: the pinned variant, else `planned` (> 0), else the choice by shape; then the fix-ups
GemmPlan plan_gemm(const jat_model* m, int site, int M, int N, int ksplit, bool folding, int planned = -1);
// the gated-residual GEMMs [M, D] = A[M, K] W^T into the residual stream: out_proj (G_OUT) and fc2 (G_FC2)
GemmPlan plan_resid(const jat_model* m, int site, int M, int K, bool folding, bool split_ws);
GemmPlan plan_qkv(const jat_model* m, int M, int K, bool folding, bool split_ws);   // [M, D + 2 kvD] ahead of the attention kernel
GemmPlan plan_patch(const jat_model* m, int rows, int K);   // the first patch-embed Linear [rows, bottleneck]
bool plan_fold_norms(const jat_model* m, int M);            // may a sampler bucket of M rows per forward fold its norms
