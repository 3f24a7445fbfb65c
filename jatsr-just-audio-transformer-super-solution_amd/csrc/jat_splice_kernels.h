// Launchers of the inverse-STFT, band-splice and long-term-spectrum kernels (splice.hip), used by jat_splice.cpp, and the
// host-made overlap-add envelope they divide by.  They run on the plan, window and twiddle tables of a jat_audio_metrics handle.
#pragma once
#include <vector>

#include "jat_metrics_kernels.h"

constexpr int SP_MAX_OVERLAP = 64;     // n_fft / hop of the inverse transform: 4 .. SP_MAX_OVERLAP
constexpr int LT_SLICES = 64;          // partial spectra per row of the long-term spectrum (JAT_LTAS_SLICES)
constexpr int LT_BINS_PER_THREAD = 9;  // 256 x 9 >= 1 + 4096 / 2

// hop divides n_fft, hop <= n_fft / 4 (the envelope is then positive on every output sample) and n_fft / hop <= SP_MAX_OVERLAP
inline bool splice_hop_ok(int n_fft, int hop) {
  return hop >= 1 && n_fft % hop == 0 && hop <= n_fft / 4 && n_fft / hop <= SP_MAX_OVERLAP;
}

// The envelope env[pos] = sum_f w[pos - f hop]^2 over the frames f in [0, frames) that cover the padded position pos.  With
// pos = q hop + r and R = n_fft / hop the covering frames are f = q - m for m in [m_lo, m_hi], m_lo = max(0, q - (frames - 1)),
// m_hi = min(R - 1, q), so the value depends on (m_lo, m_hi, r) alone:
//   table[(m_hi (m_hi + 1) / 2 + m_lo) hop + r] = sum_{m = m_lo}^{m_hi} w[r + m hop]^2        (fp64 sums, stored fp32)
// Row (0, R - 1) is the interior, periodic in hop; rows (0, m_hi < R - 1) are the head, rows (m_lo > 0, R - 1) the tail, and
// the remaining rows serve signals of fewer than R frames, where both ends are cut.  R (R + 1) / 2 rows of hop values.
void splice_envelope_table(int n_fft, int hop, std::vector<float>* table);

size_t splice_lds_bytes(const MetricsPlan& p);
// blocks of the splice transform kernel one CU holds at once with this plan's LDS
hipError_t splice_blocks_per_cu(const MetricsPlan& p, int* blocks);

// X complex64 [B, bins, frames] -> W fp32 [B, frames, n_fft]: W[b, f, i] = w[i] irfft(X[b, :, f])[i], two frames per transform
hipError_t istft_frames_launch(const MetricsPlan& p, const MetricsTables& t, int slots, const float2* X, int B, int frames,
                               float* W, hipStream_t s);
// W[b, f, i] = w[i] irfft(a rfft(w (src - gen) of frame f))[i] with the rows cut to n samples, two frames per transform;
// gen [B, L_gen], src [B, L_src], gain a [bins]
hipError_t splice_frames_launch(const MetricsPlan& p, const MetricsTables& t, int slots, const float* gen, const float* src,
                                int B, int64_t L_gen, int64_t L_src, int n, int frames, const float* gain, float* W,
                                hipStream_t s);
// out[b, t] = (sum over the covering frames, ascending, of W[b, f, t + n_fft / 2 - f hop]) / env, for t < n; with gen
// (rows of L_out samples) the quotient is added to gen[b, t], and out[b, t] = gen[b, t] for t in [n, L_out).  out [B, L_out].
hipError_t overlap_add_launch(const MetricsPlan& p, const float* W, const float* envelope, int B, int frames, int n,
                              const float* gen, int64_t L_out, float* out, hipStream_t s);
// x fp32 [B, L] -> P fp64 [B, bins] = mean over frames of |X[k, f]|^2; partial: B * LT_SLICES * bins doubles
hipError_t ltas_launch(const MetricsPlan& p, const MetricsTables& t, const float* x, int B, int L, int frames, double* partial,
                       double* P, hipStream_t s);
