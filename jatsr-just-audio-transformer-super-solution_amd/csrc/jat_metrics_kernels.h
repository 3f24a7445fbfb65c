// Launchers of the audio-metric kernels (metrics.hip), used by jat_metrics.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int MT_THREADS = 256;        // one STFT block: 4 waves
constexpr int MT_GROUP_POINTS = 1024;  // frames transformed side by side in one block: max(1, MT_GROUP_POINTS / n_fft)
constexpr int MT_MAX_PASSES = 6;       // radix-4 passes of a 4096-point transform
constexpr int MT_SLICES = 64;          // partial sums per row in the finishing stage
constexpr int MT_W_PER_THREAD = 16;    // band weights a thread carries to LDS: 256 x 16 >= 4096 - 2

// One transform size: Stockham autosort, radix 4 with one closing radix-2 pass when log2(n_fft) is odd.  The first
// pass (no twiddles) runs on the samples as they are loaded; pass p >= 1 reads its twiddles at tw[off[p] + (r - 1) * ns[p] + k].
struct MetricsPlan {
  int n_fft = 0, hop = 0, bins = 0, n_mels = 0;
  int group = 1;                       // frames per group
  int n_pass = 0;                      // passes including the first
  int radix[MT_MAX_PASSES] = {}, ns[MT_MAX_PASSES] = {}, off[MT_MAX_PASSES] = {};
  int n_tw = 0;                        // float2 entries of the twiddle table
  int nnz = 0;                         // non-zero filterbank weights
  int slots = 1;                       // blocks the device holds at once: CUs x blocks per CU by LDS and registers
};

// device tables of one handle
struct MetricsTables {
  const float* window = nullptr;       // [n_fft] periodic Hann
  const float2* tw = nullptr;          // [n_tw]
  const int* band_first = nullptr;     // [n_mels] first bin of the band
  const int* band_count = nullptr;     // [n_mels] bins of the band
  const int* band_off = nullptr;       // [n_mels] offset of its weights
  const float* band_w = nullptr;       // the non-zero weights, band after band
};

// what a jat_audio_metrics handle owns (jat_metrics.cpp creates and destroys it; jat_splice.cpp uses it as well)
struct jat_audio_metrics {
  MetricsPlan plan;
  MetricsTables tab;
  void* dev = nullptr;                 // one allocation behind every table
  const float* envelope = nullptr;     // overlap-add envelope table of jat_splice_kernels.h; null when hop does not allow it
  int splice_slots = 1;                // blocks of the splice transform kernel the device holds at once
};

// frame groups one block runs through, and the blocks per row that follow from it; a result never depends on it
int metrics_groups_per_block(const MetricsPlan& p, int B, int frames);
inline int metrics_blocks_per_row(const MetricsPlan& p, int B, int frames) {
  const int fpb = p.group * metrics_groups_per_block(p, B, frames);
  return (frames + fpb - 1) / fpb;
}
size_t metrics_lds_bytes(const MetricsPlan& p);
// blocks of the STFT kernel one CU holds at once with this plan's LDS (the runtime's occupancy figure)
hipError_t metrics_blocks_per_cu(const MetricsPlan& p, int* blocks);

// The STFT-and-reduce pass over rows pred[b], gt[b] (fp32 [B, L]).  Each of the outputs may be null:
//   mel_pow  [B, 2, frames, n_mels]  mel power of pred (0) and gt (1);  block_max [B, 2, blocks per row] its maxima
//   lsd_frames [B, frames]
//   Xp, Xg   [B, bins, frames] the two spectra (unit tests)
hipError_t metrics_stft_launch(const MetricsPlan& p, const MetricsTables& t, const float* pred, const float* gt, int B, int L,
                               int frames, float* mel_pow, float* block_max, float* lsd_frames, float2* Xp, float2* Xg,
                               hipStream_t s);
// dB conversion, the -80 dB floor and the sums: partial [B, MT_SLICES, 3] doubles, out [B, 3] doubles (lsd_db, mel_l1, mel_l2);
// pred_db / gt_db [B, n_mels, frames] or null; lsd_frames null when no LSD was asked for, mel_pow null when n_mels == 0
hipError_t metrics_finish_launch(const MetricsPlan& p, const float* mel_pow, const float* block_max, int blocks_per_row,
                                 const float* lsd_frames, int B, int frames, double* partial, double* out, float* pred_db,
                                 float* gt_db, hipStream_t s);
