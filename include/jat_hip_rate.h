/*
 * jat_hip_rate.h — C ABI of the voicing-aware index rates, an addition to jat_hip.h: the index rate of the
 * retrieval blend as a per-frame track derived from a pitch track, in the place of one scalar for a whole file.  It carries
 * RVC's `protect` (unvoiced frames get only a share of the retrieved feature) and the reference roadmap's F0-stability
 * classes.  The conventions of jat_hip.h hold: device pointers unless marked [host], fp32 in both operand-dtype builds, every
 * call only enqueues on the caller's stream, none of them synchronises, allocates or copies between host and device, and each
 * may be captured into a graph ([host] arrays are read before the call returns).  A refused call returns JAT_E_INVALID,
 * launches nothing and writes nothing.  No kernel uses atomics: the bits repeat from run to run and depend on neither B nor
 * the grid.
 *
 * Definitions
 *   Live.  Frame j of a pitch track is LIVE when voiced[j] != 0 and f0[j] is positive and finite (the VOICED of
 *     jat_hip_harm.h); anything else is not live and never faults.
 *   Classes.  For a live frame t, count[t] is the number of j in [max(0, t - W), min(F - 1, t + W)], t itself included, with
 *     j live, f0[j] <= f0[t] * ratio and f0[t] <= f0[j] * ratio; each product is one fp32 multiply rounded once (no logarithm).
 *     count[t] = 0 on a frame that is not live.  cls[t] = 0 (not live), 1 (live, count < min_count: unstable) or 2 (live,
 *     count >= min_count: stable).  summary[b] = {live frames, stable frames} of row b, integers.
 *   Rate track.  c[t] = rates[min(cls[t], 2)] for t < F; frames the pitch track does not reach are unvoiced, c[t] = rates[0]
 *     for t >= F.  With a = max(0, t - S), b = min(T - 1, t + S), n = b - a + 1,
 *       r[t] = clamp(c[t] + (((c[a] - c[t]) + (c[a+1] - c[t])) + ... + (c[b] - c[t])) / float(n), 0, 1),
 *     every difference, add and the division rounded once.  The mean is taken of differences, so a frame farther than S from
 *     any change of class carries its class's rate exactly, and a constant class row gives a constant rate row.  S = 0 gives c.
 *     A rate of -0 is taken as +0.
 *   Mix.  y[b, c, t] = fma(1 - r, x[b, c, t], r * v[b, c, t]) with r = rates[b, t]: 1 - r and r * v are each rounded once, then
 *     one fma.  A track whose entries all equal R gives the bits jat_bank_blend, jat_bank_blend_topk and jat_bank_mix_scales
 *     give at rate R from the same x and the same retrieved v, where v is what those calls return at rate 1 (fma(0, x, 1 v):
 *     for finite x it is v, except that a v of -0 becomes +0 where x > 0 or x is +0, and exactly there the sign of that zero
 *     cannot reach the final sum).  The device does not check that rates lies in [0, 1].
 */
#ifndef JAT_HIP_RATE_H
#define JAT_HIP_RATE_H

#include "jat_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define JAT_RATE_MAX_HALF_WINDOW 32
#define JAT_RATE_MAX_SMOOTH 16

/* f0 fp32 [B, F] and voiced uint8 [B, F] as jat_yin / jat_pyin_track write them -> cls uint8 [B, F]; count int32 [B, F] (may be
 * NULL); summary int32 [B, 2] (may be NULL).  JAT_E_INVALID: a null f0, voiced or cls, B outside 1..65535, F < 1, half_window
 * outside 0..32, ratio not finite or <= 1, min_count outside 1..2 half_window + 1. */
int jat_f0_classes(const float* f0, const uint8_t* voiced, int32_t B, int32_t F, int32_t half_window, float ratio,
                   int32_t min_count, uint8_t* cls, int32_t* count, int32_t* summary, void* stream);

/* cls uint8 [B, F] (a value above 2 counts as 2) -> r fp32 [B, T].  [host] rates[3] = {unvoiced, unstable, stable}.
 * JAT_E_INVALID: a null buffer, B outside 1..65535, F < 1, T < 1, smooth outside 0..16, a rate outside [0, 1] or not finite. */
int jat_rate_track(const uint8_t* cls, int32_t B, int32_t F, int32_t T, const float* rates, int32_t smooth, float* r,
                   void* stream);

/* x, v fp32 [B, C, T], rates fp32 [B, T] -> y fp32 [B, C, T]; y may be x or v (any other overlap of y with an input is
 * refused).  JAT_E_INVALID: a null buffer, B outside 1..65535, C < 1, T < 1, y overlapping x, v or rates otherwise. */
int jat_rate_mix(const float* x, const float* v, const float* rates, float* y, int32_t B, int32_t C, int32_t T, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* JAT_HIP_RATE_H */
