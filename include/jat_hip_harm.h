/*
 * jat_hip_harm.h — C ABI of the F0-guided harmonic analysis, the harmonic template and the harmonic comparison
 * (DESIGN.md §25), an addition to jat_hip.h.  The conventions of jat_hip.h hold: device pointers unless marked [host], fp32
 * in both operand-dtype builds, every call only enqueues on the caller's stream, none synchronises, allocates or copies
 * between host and device, and each may be captured into a graph.  tests/harmonic_ref.py states the definitions in fp64.
 *
 * Definitions
 *   Common.  The framing of jat_yin: frames = 1 + L / hop_length, frame f is x_pad[f hop : f hop + N] with N / 2 zeros a side
 *     of the row, N = frame_length even and in 16..8192.  w[n] = float(0.5 - 0.5 cos(2 pi n / N)) is the periodic Hann window
 *     (the fp64 formula of jat_audio_metrics_create, rounded to fp32).  H = n_harmonics in 1..JAT_HARM_MAX.
 *     Phases are fixed-point turns in uint32:  turns(f) = uint32(llrint(f / sr * 2^32)), the quotient and the product in
 *     fp64.  All phase arithmetic is integer arithmetic modulo 2^32: exact, whatever the order of summation.  The angle handed
 *     to sine and cosine is  angle(p) = 2 pi float(int32(p)) 2^-32  in [-pi, pi), float() rounding to nearest even.
 *     A frame is VOICED when its flag is set and its f0 is positive and finite; anything else is unvoiced and never faults.
 *   Analysis.  Harmonic h = 1 .. H of frame f is LIVE when the frame is voiced and 0 < h f0 < sr / 2 - 2 sr / N (fp64; the
 *     guard is the half-width of the Hann main lobe).  For a live harmonic
 *         s = turns(h f0),  p_n = (s n) mod 2^32,  c = sum_n w[n] x_f[n] exp(-i angle(p_n)),  amp = 2 |c| / sum_n w[n]
 *     (the kernel divides by N / 2, the sum of the exact window; the rounded window's sum differs from it by less than
 *     2^-25 of it, which the tests' bound carries).  A harmonic that is not live gets 0 and no sample is read for it.
 *     energy = sum_n (w[n] x_f[n])^2 for every frame.  Every sum runs in ONE order: lane l of a 64-lane wave adds the terms
 *     n = l, l + 64, .. in ascending n with one fma each, then the 64 partial sums are added in a butterfly (lane ^ 32, 16,
 *     8, 4, 2, 1).  No atomics: the bits are the same from run to run, for a row alone or in a batch, whatever the grid.
 *   Synthesis.  For sample n of a row: f = n / hop, u = (n - f hop) / hop (fp64), frame f + 1 clamped to the last frame.
 *     With v_f "frame f is voiced":  f0(n) = (1 - u) f0_f + u f0_{f+1} (fp64) when both are voiced, the voiced one's f0 when
 *     one is, 0 when none is;  a_h(n) = (1 - u) (v_f ? amp_{f,h} : 0) + u (v_{f+1} ? amp_{f+1,h} : 0) in fp32 with u rounded
 *     to fp32;  inc[n] = turns(f0(n)) (0 when f0(n) is not below sr / 2);  phase[n] = sum_{m < n} inc[m] mod 2^32, phase[0] = 0;
 *         y[n] = sum_{h ascending} a_h(n) sin(angle((h phase[n]) mod 2^32)),
 *     without the terms that have h f0(n) >= sr / 2 (no aliasing).  The prefix is an integer scan (per-frame sums, a scan
 *     over frames, the prefix inside the frame): it does not depend on how it is split and equals numpy's uint32 cumsum.
 *   Comparison.  A cell (f, h) counts when frame f of the reference is voiced and amp_ref > floor;
 *     e = 20 log10((amp_a + floor) / (amp_ref + floor)) in fp64.  Cells with h f0_ref < cutoff_hz (fp64) form the KEPT band,
 *     the others the REGENERATED band.  out[b] = {n, sum e, sum e^2, sum |e|} of the kept band, then of the regenerated band.
 *     One block per row: thread t adds the cells t, t + 256, .. of the row's [frames, H] table in order, then a tree over
 *     the threads, as jat_f0_compare does.
 */
#ifndef JAT_HIP_HARM_H
#define JAT_HIP_HARM_H

#include "jat_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define JAT_HARM_MAX 128   /* harmonics of one call at most */

/* x fp32 [B, L], f0 fp32 and voiced uint8 [B, frames] -> amp fp32 [B, frames, H], energy fp32 [B, frames] (may be NULL).
 * frames must be 1 + L / hop_length (JAT_E_INVALID otherwise); B in 1..65535; frames * H must fit 31 bits. */
int jat_harmonic_analyze(const float* x, int32_t B, int64_t L, const float* f0, const uint8_t* voiced, int32_t frames,
                         int32_t n_harmonics, int32_t sr, int32_t frame_length, int32_t hop_length, float* amp, float* energy,
                         void* stream);

/* bytes of the scan's workspace for jat_harmonic_synth at (B, L, hop_length): one uint32 per frame [host] */
int jat_harmonic_synth_workspace_bytes(int32_t B, int64_t L, int32_t hop_length, size_t* bytes);

/* f0 fp32, voiced uint8 [B, frames], amp fp32 [B, frames, H] -> y fp32 [B, L]; phase uint32 [B, L] (a test output, may be
 * NULL).  frames must be 1 + L / hop_length.  workspace: at least jat_harmonic_synth_workspace_bytes bytes, 4-byte aligned,
 * the caller's (JAT_E_INVALID when too small); its contents are scratch. */
int jat_harmonic_synth(const float* f0, const uint8_t* voiced, const float* amp, int32_t B, int32_t frames,
                       int32_t n_harmonics, int64_t L, int32_t sr, int32_t hop_length, float* y, uint32_t* phase,
                       void* workspace, size_t workspace_bytes, void* stream);

/* amp_a, amp_ref fp32 [B, frames, H], f0_ref fp32 and voiced_ref uint8 [B, frames] -> out fp64 [B, 8] as defined above.
 * cutoff_hz >= 0 or +infinity (every cell is kept), floor > 0 and finite. */
int jat_harmonic_compare(const float* amp_a, const float* amp_ref, const float* f0_ref, const uint8_t* voiced_ref, int32_t B,
                         int32_t frames, int32_t n_harmonics, double cutoff_hz, double floor, double* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* JAT_HIP_HARM_H */
