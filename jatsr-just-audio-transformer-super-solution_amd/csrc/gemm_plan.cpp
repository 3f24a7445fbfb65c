// Variant choice and K-split planning (gemm_plan.h): host arithmetic on shapes, the variant table and the model's switches.
#include "gemm_plan.h"

#include <cstdlib>

#include "gemm_variants.h"

static int env_switch(const char* name) { const char* v = getenv(name); return v ? atoi(v) : 1; }

// Tile choice by shape (gemm_variants.h; measured on MI355X, profiles/r01/gemm_variants.md).  What
// decides is how the tile count quantises onto 256 CUs (one 8-wave block or two 4-wave blocks per CU) and how
// many bytes are staged per MFMA: 256x160 with DMA waves (variant 25; 224 tiles at M=7168, N=1280: one round) >
// 128x160 > 256x256 > 128x128.
int pick_variant(int M, int N, int nbatch) {
  // score = in-tile efficiency factor x tile-quantisation efficiency on the slots the variant occupies
  // (256 CUs x 1 eight/twelve-wave block, or x 2 four-wave blocks); factors calibrated on the measured block GEMMs
  // at M = 7168 and M = 3584 (profiles/r01/gemm_variants_*.log).  Multi-round 1-block-per-CU variants pay 15 %:
  // their prologue/epilogue is not overlapped by a co-resident block.
  int best = V_128x128, best_pick = 0;
  double best_score = -1.0;
  for (const GemmVariant& c : kGemmVariants) {
    if (!c.pick || N % c.bn() != 0) continue;
    const long t = (long)((M + c.bm() - 1) / c.bm()) * (N / c.bn()) * nbatch;
    const long rounds = (t + c.slots() - 1) / c.slots();
    double score = c.score * (double)t / (double)(rounds * c.slots());
    // multi-round penalty: the 12-wave DMA-wave variants (25, 26) pay their un-overlapped prologue/epilogue per round;
    // the 8-wave tiles (21, 31-35) less so (M = 9660, N = 5120: 110 us vs 124 us for 128x160, tools/gemm_shapes_bench.py)
    if (rounds > 1 && (c.id == V_DMA_256x160 || c.id == V_DMA_256x128)) score *= 0.85;
    // padding waste of a ragged last row tile counts against big tiles
    score *= (double)M / (double)(((M + c.bm() - 1) / c.bm()) * c.bm());
    if (score > best_score || (score == best_score && c.pick < best_pick)) { best_score = score; best = c.id; best_pick = c.pick; }
  }
  // a half-size batch's QKV GEMM (M = 3584, N = 1792): 392 tiles of 128 x 128 fill 77 % of the 512 four-wave slots; 196 tiles of
  // 256 x 128 with the DMA-wave pipeline are one block on 196 CUs and measured faster (forward 5.530 -> 5.455 ms,
  // profiles/r03/forward_B28_out_qkv_tile_sweep.log).  Only where those tiles make one nearly full round.
  if (best == V_128x128 && nbatch == 1 && N % 128 == 0) {
    const long t26 = (long)((M + 255) / 256) * (N / 128);
    if (t26 >= 192 && t26 <= 256 && M % 256 == 0) best = V_DMA_256x128;
  }
  // 36: the tile of 31 with the software-pipelined bf16 / GELU epilogue (JAT_EPI_PIPE=0 keeps the plain one: A/B)
  static const int epi_pipe = env_switch("JAT_EPI_PIPE");
  if (epi_pipe && best == V_PP_224x320) best = V_PP_224x320_EPI;
  // 39: the k-step-pair 224 x 160 tile for the N = 1280 class when it fills more of the chip than 256 x 160 (M = 7168: 256 tiles
  // against 224); launch_gemm falls back to 32 for anything but the split-residual producer epilogues.  JAT_KPAIR=0: A/B
  static const int kpair = env_switch("JAT_KPAIR");
  if (kpair && best == V_PP_256x160 && nbatch == 1 && M % 224 == 0 && N % 160 == 0) {
    auto eff = [](long t) { return (double)t / (double)(((t + 255) / 256) * 256); };
    if (eff((long)(M / 224) * (N / 160)) > eff((long)((M + 255) / 256) * (N / 160))) best = V_KPAIR;
  }
  // 38: the persistent two-tile form of 36 (launch_gemm falls back to 36 for shapes / epilogues it does not take); JAT_PERSIST=0: A/B
  static const int persist = env_switch("JAT_PERSIST");
  if (persist && best == V_PP_224x320_EPI && M % 224 == 0 && (long)(M / 224) * (N / 320) * nbatch > 256) best = V_PERSIST;
  return best;
}

int k_slices(long tiles, int slots, int cap, int K, int min_depth) {
  int split = slots / tiles < cap ? (int)(slots / tiles) : cap;
  while (split > 1 && ((K / 64) % split != 0 || K / split < min_depth)) --split;
  return split > 1 ? split : 1;
}

// slices of [M, N] (at least 256 deep) on the tiles of variant v
static int k_slices_on(int v, int M, int N, int cap, int K) {
  const GemmVariant& t = *gemm_variant(v);
  return k_slices((long)((M + t.bm() - 1) / t.bm()) * (N / t.bn()), t.slots(), cap, K, 256);
}

// pinned (JAT_GEMM_VARIANT(S)) > planned > by shape; an unknown pinned id passes through: launch_gemm rejects it
GemmPlan plan_gemm(const jat_model* m, int site, int M, int N, int ksplit, bool folding, int planned) {
  if (ksplit < 1) ksplit = 1;
  int v = m->variants[site] >= 0 ? m->variants[site] : planned > 0 ? planned : pick_variant(M, N, ksplit);
  const GemmVariant* t = gemm_variant(v);
  if (folding && t && !t->coalesced()) t = gemm_variant(v = V_128x128);   // folding lives in the coalesced epilogues
  if (t && N % t->bn() != 0) v = V_128x128;                               // N must divide the tile
  return {v, ksplit};
}

GemmPlan plan_resid(const jat_model* m, int site, int M, int K, bool folding, bool split_ws) {
  const int D = m->D;
  if (!split_ws || folding || K < 1024 || m->variants[site] >= 0) return plan_gemm(m, site, M, D, 1, folding);
  // Which tile the slices are cut for: 64 x 128 tiles (what pick_variant takes un-split) are bound by the per-CU L2->LDS rate
  // (24 KB per K-tile and block, two blocks per CU); 128 x 128 tiles move 2/3 of the bytes per flop and, cut into more slices,
  // give as many blocks.  Measured per 50-step run (B = 2 / 4 / 8): fc2 133.0 -> 130.3, 169.0 -> 154.5, 253.6 -> 220.1 ms (B = 1:
  // neutral); out_proj only pays from M = 2048 (B = 8: 219.7 -> 212.8 ms).
  // (The slices are launched on the tile pick_variant takes for M x D x slices, which need not be the one they were cut for.)
  if (M <= kSplitMaxRows)
    return plan_gemm(m, site, M, D, k_slices_on((K >= 4096 || M >= 1536) ? V_128x128 : pick_variant(M, D), M, D, kSplitMax, K), false);
  // a mid-size un-folded bucket (a T = 4096 file: M = 2760): the 64 x 128 tiles that fill the chip un-split are bound by the
  // per-CU L2->LDS rate (24 KB per K-tile and block, two blocks per CU); for the long-K fc2 two slices of 128 x 128 tiles
  // (the same 440 blocks, 2/3 of the bytes per flop) + the finishing pass are faster: 70 -> 45 us
  // A half-size batch (configs[1]'s single forward, M = 3584): the 224 x 160 k-step-pair tile makes 128 tiles — two K slices
  // put one on every CU (tile bytes per flop: 0.011 against 0.022 for the 64 x 160 tiles that fill the chip un-split); the
  // finishing pass also applies the norm that follows, which saves the separate norm launch.  JAT_KPAIR_SPLIT=0: A/B
  static const int kpair_split = env_switch("JAT_KPAIR_SPLIT");
  if (kpair_split && M % 224 == 0 && D % 160 == 0) {
    const int tiles = (M / 224) * (D / 160);
    const int split = k_slices(tiles, 256, 2, K, 512);   // the workspace of this bucket holds two slices (split_ws_slices)
    // only where the slices fill the chip (M = 3136 ... 3584: 224 ... 256 blocks); below that the 128 x 128 slices stay (measured
    // at M = 3584 only: profiles/r03/forward_B28_kernel_table_kpair_split.txt)
    if (split > 1 && tiles * split >= 224 && (K >= 4096 || kpair_split >= 2)) return plan_gemm(m, site, M, D, split, false, V_KPAIR);
  }
  return plan_gemm(m, site, M, D, K >= 4096 ? k_slices_on(V_128x128, M, D, 2, K) : 1, false);
}

// K-slices for the QKV GEMM of a small bucket (M <= kSplitMaxRows, un-folded, separate attention kernel): its 56 tiles at one
// chunk leave 200 CUs without weights to pull; the slices are summed, rotated and laid out by splitk_qkv_finish_kernel
GemmPlan plan_qkv(const jat_model* m, int M, int K, bool folding, bool split_ws) {
  const int N = m->D + 2 * m->kvD;
  int ksplit = 1;
  if (m->sw.qkv_split && m->D % 64 == 0 && m->kvD % 64 == 0 && split_ws && !folding && M <= kSplitMaxRows && m->variants[G_QKV] < 0) {
    const int v = pick_variant(M, N);
    if (N % gemm_variant(v)->bn() == 0) ksplit = k_slices_on(v, M, N, kSplitMax, K);
  }
  return plan_gemm(m, G_QKV, M, N, ksplit, folding);
}

// The first patch-embed Linear is narrow and deep ([rows, 4096 or 8192] x [512, .]^T: 64 x 128 tiles make at most one 4-wave
// block per CU at the bench's batch, each walking 64-128 K-tiles): K slices put two blocks on every CU, the finishing pass
// adds bias and GELU (same expression as the epilogue).  The partials live in the MLP hidden buffer, idle until block 0's fc1.
GemmPlan plan_patch(const jat_model* m, int rows, int K) {
  int ksplit = 1;
  if (m->sw.patch_split && m->variants[G_OTHER] < 0 && m->bott % 128 == 0) {
    const int tiles = ((rows + 63) / 64) * (m->bott / 128);
    // measured (profiles/r03/patch_embed_split_ab.log): pays for the single forward (K = 8192: 5.45 -> 5.41 ms) and for one chunk
    // (24 tiles: 133.4 -> 131.9 ms), not for the sampler's half-depth form at the bench's batch (224 tiles, K = 4096: 353.1 vs 353.6 ms)
    if (!(tiles > 128 && K < 8192)) {
      const int cap = m->mlp / (2 * m->bott);   // partial slices must fit the MLP hidden buffer: split * bott * 4 <= mlp * 2 bytes per row
      ksplit = k_slices(tiles, 512, cap < 4 ? cap : 4, K, 1024);
    }
  }
  return plan_gemm(m, G_OTHER, rows, m->bott, ksplit, false);   // this Linear neither produces nor consumes folded norms
}

// Norm folding (RMSNorm models; the "fold_norm" switch: 0 off, 1 buckets above kSplitMaxRows, 2 every bucket).  The consumer
// side reads the row partials lane-linear: needs 4, 8 or 16 slots per row; the three producers of the residual stream (patch
// embed, out_proj, fc2: all [M, D]) must agree on the slot count and have the coalesced epilogue.
bool plan_fold_norms(const jat_model* m, int M) {
  if (m->sw.fold_norm <= 0 || m->cfg.norm_mode != JAT_NORM_RMS_W || !m->fold_src_ok) return false;
  if (M <= kSplitMaxRows && m->sw.fold_norm < 2) return false;   // small-M buckets finish fc2 / out_proj with split-K instead (2: force, tests)
  int wave_n = 0;
  for (int site : {G_OUT, G_FC2, G_OTHER}) {
    const GemmVariant* t = gemm_variant(m->variants[site] >= 0 ? m->variants[site] : pick_variant(M, m->D));
    if (!t || !t->coalesced() || (wave_n && t->wave_n() != wave_n)) return false;
    wave_n = t->wave_n();
  }
  const int np = m->D / wave_n;
  return np == 4 || np == 8 || np == 16;
}
