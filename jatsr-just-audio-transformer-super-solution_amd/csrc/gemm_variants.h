// The GEMM tile variants: one row per live instantiation of the kernel template.  Plain C++: gemm.hip instantiates its
// kernels from these rows (launch_gemm), gemm_plan.cpp chooses among them; nothing else describes a variant.
#pragma once

// the ids the host code names
enum GemmVariantId : int {
  V_LAST_RESORT = 10,  // the only tile for N % 128 != 0 (N % 64 == 0); no model that passes jat_model_create produces one
  V_128x128 = 20,      // valid for every N the models have: what the fix-ups and the split-K slices fall back on
  V_DMA_256x160 = 25, V_DMA_256x128 = 26, V_PP_224x320 = 31, V_PP_256x160 = 32, V_PP_224x320_EPI = 36, V_PERSIST = 38, V_KPAIR = 39,
};

struct GemmVariant {
  int id;
  int WM, WN, TM, TN, PIPE, CE;   // template arguments of gemm_bf16_kernel: waves and 16 x 16 MFMA tiles per wave along M / N,
                                  // main loop, epilogue (0 plain, 1 coalesced, 2 coalesced + software-pipelined bf16 / GELU)
  int fallback;                   // -1, or the id launched instead for the shapes / epilogues the variant's own kernel does not take
  int blocks_per_cu;              // co-resident blocks (the kernel's launch bounds): the chooser counts 256 x this many slots
  double score;                   // the chooser's in-tile efficiency factor (gemm_plan.cpp: pick_variant)
  int pick;                       // 0: never chosen by shape; else the chooser's precedence (equal scores: the lower one wins)

  constexpr int bm() const { return WM * TM * 16; }   // the tile: BM x BN
  constexpr int bn() const { return WN * TN * 16; }
  constexpr int wave_n() const { return TN * 16; }   // columns per wave tile: the slot width of the norm-folding row partials
  constexpr bool coalesced() const { return CE != 0; }
  constexpr int slots() const { return 256 * blocks_per_cu; }
};

// Ids are stable (bench.py keys, profiles/ and DESIGN.md cite them); an id without a row is retired and rejected: 0-9 (PIPE 0 / 1),
// 11-17 (PIPE 2 without the coalesced epilogue, PIPE 3), 19, 22-24 (PIPE 4 / 5), 29-30 (PIPE 7), 37 (pipelined split-residual
// epilogue: slower, profiles/r03).
// 10 and 34 are reached through the per-kernel entry points and a pinned JAT_GEMM_VARIANT only; 36, 38 and 39 replace a
// chosen 31 / 36 / 32 (pick_variant's closing rules), so they carry no score of their own.
// 38 and 39 run kernels of their own (gemm_persist_kernel on the tile of 36; gemm_kpair_kernel on a 224 x 160 tile) and carry
// the row of their fallback: the planner therefore sees 39 as the 256 x 160 tile of 32, not as the 224 x 160 its kernel walks.
inline constexpr GemmVariant kGemmVariants[] = {
    // id  WM WN TM TN PIPE CE  fallback  blocks/CU  score  pick
    {10,   2, 2, 4, 2, 1,  0,  -1,       2,         0.00,  0},   // 128 x  64  PIPE 1, plain epilogue
    {18,   2, 2, 4, 5, 2,  1,  -1,       2,         0.95,  2},   // 128 x 160  PIPE 2 + coalesced epilogue
    {20,   2, 2, 4, 4, 2,  1,  -1,       2,         0.95,  1},   // 128 x 128
    {21,   2, 4, 8, 4, 2,  1,  -1,       1,         1.00,  5},   // 256 x 256
    {25,   4, 2, 4, 5, 6,  1,  -1,       1,         1.00,  3},   // 256 x 160  PIPE 6: 8 MFMA waves + 4 DMA waves
    {26,   4, 2, 4, 4, 6,  1,  -1,       1,         0.90,  4},   // 256 x 128
    {27,   2, 2, 2, 5, 2,  1,  -1,       2,         0.60,  6},   //  64 x 160  small-M tiles (PIPE 2)
    {28,   2, 2, 2, 4, 2,  1,  -1,       2,         0.62,  7},   //  64 x 128
    {31,   2, 4, 7, 5, 8,  1,  -1,       1,         1.12,  8},   // 224 x 320  PIPE 8: quadrant ping-pong, 2 LDS stages; factors
    {32,   4, 2, 4, 5, 8,  1,  -1,       1,         1.01,  9},   // 256 x 160    calibrated on profiles/r02/gemm_variants_*.log
    {33,   2, 4, 8, 4, 8,  1,  -1,       1,         1.06, 10},   // 256 x 256
    {34,   2, 4, 4, 7, 8,  1,  -1,       1,         0.00,  0},   // 128 x 448
    {35,   2, 4, 7, 4, 8,  1,  -1,       1,         1.06, 11},   // 224 x 256
    {36,   2, 4, 7, 5, 8,  2,  -1,       1,         0.00,  0},   // 224 x 320  the tile of 31 with the software-pipelined epilogue
    {38,   2, 4, 7, 5, 8,  2,  36,       1,         0.00,  0},   // persistent two-tile form of 36
    {39,   4, 2, 4, 5, 8,  1,  32,       1,         0.00,  0},   // k-step-pair 224 x 160 tile for the split-residual producers
};
inline constexpr int kNumGemmVariants = (int)(sizeof(kGemmVariants) / sizeof(kGemmVariants[0]));

// the row of a live id, nullptr for a retired or unknown one
constexpr const GemmVariant* gemm_variant(int id) {
  for (const GemmVariant& v : kGemmVariants)
    if (v.id == id) return &v;
  return nullptr;
}
