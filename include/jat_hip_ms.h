/*
 * jat_hip_ms.h — C ABI of multi-scale latent retrieval, an addition to jat_hip.h: one bank per time scale
 * s in {1, 2, 4, 8}, the prediction pooled to that scale, looked up with the search and blend of jat_hip.h, brought back to
 * the frame rate by linear interpolation and mixed in.  The conventions of jat_hip.h hold: device pointers unless marked
 * [host], fp32, every call only enqueues on the caller's stream, none of the three synchronises, allocates or copies between
 * host and device, and each may be captured into a graph.
 *
 * Definitions (every operation fp32, rounded to nearest even, nothing fused but the last line of the mix)
 *   Pooling.  With q_j = (src_j - mean[c]) / std[c] (the channel affine of jat_hip.h), the window of scale s that starts at
 *     frame f of a source of length len holds cnt = min(s, len - f) frames and pools to
 *         p = (((q_f + q_{f+1}) + q_{f+2}) + ...) / float(cnt)
 *     (ascending sequential adds, then one division).  s = 1 is q_f itself, bit for bit.  Bank rows and queries pool alike.
 *   Interpolation.  A track v [B, C, Ts], Ts = ceil(T / s), is read at frame t as u = v[t] for s = 1 and otherwise
 *         p = (t + 0.5) / s - 0.5,  j0 = floor(p),  w = p - j0  (a dyadic fraction, exact),
 *         ja = clamp(j0, 0, Ts - 1),  jb = clamp(j0 + 1, 0, Ts - 1),  u = (1 - w) v[ja] + w v[jb]:
 *     linear interpolation with half-pixel centres (torch's F.interpolate(mode="linear", align_corners=False) at scale
 *     factor s where T is a multiple of s).
 *   Mix.  m = -0.0f; for i ascending m = m + a_i u_i (product and sum each rounded);  y = fma(1 - rate, x, rate m): the product
 *     rate m rounded, then ONE fused multiply-add.  That is what the last line of jat_bank_blend computes as it is compiled, and
 *     it is the only fused operation here; rate 0 returns x, rate 1 returns m.
 */
#ifndef JAT_HIP_MS_H
#define JAT_HIP_MS_H

#include "jat_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define JAT_BANK_MAX_SCALES 4   /* scales of one mix at most; each is 1, 2, 4 or 8 */

/* jat_bank_add with a window: row size + i holds, per channel, the pooled value (above) of the window of `window` frames that
 * starts at frame first + i stride of the [channels, len] source, cut by the end of the source; then fp16, and the norms as
 * jat_bank_add computes them.  window in {1, 2, 4, 8}; window = 1 writes what jat_bank_add writes, bit for bit.  A paired
 * bank pools key_src and value_src alike, each under its statistics.  Every window START lies inside the source
 * (JAT_E_INVALID otherwise); JAT_E_STATE, with the bank as it was, when size + count > capacity. */
int jat_bank_add_pooled(jat_bank* bank, const void* key_src, const void* value_src, int32_t src_is_fp16, int64_t len,
                        int64_t first, int64_t stride, int32_t count, int32_t window, const float* key_mean,
                        const float* key_std, const float* value_mean, const float* value_std, void* stream);

/* Pools x [B, C, T] at n scales in one launch that reads x once: outs[i] [B, C, ceil(T / scales[i])] holds at (b, c, ts) the
 * pooled value (above) of the window that starts at frame ts scales[i] of x[b, c, :], the last window of a row cut by the
 * row's end.  mean / std: both given (x is normalised first, as the search does) or both NULL.  scales [host]: n of 2, 4, 8,
 * strictly ascending, 1 <= n <= 3 (scale 1 needs no buffer: the search takes x and the statistics directly).  outs [host]:
 * n device pointers, none of them overlapping x.  C: a multiple of 32 in 32..1024.  The pointers and scales travel in the
 * kernel's arguments. */
int jat_bank_pool_frames(const float* x, const float* mean, const float* std, int32_t B, int32_t C, int32_t T, int32_t n,
                         const int32_t* scales, float* const* outs, void* stream);

/* y [B, C, T] = (1 - rate) x + rate sum_i weights[i] interp(tracks[i]) as defined above.  scales [host]: n of 1, 2, 4, 8,
 * strictly ascending, 1 <= n <= JAT_BANK_MAX_SCALES; tracks [host]: n device pointers, tracks[i] [B, C, ceil(T / scales[i])];
 * weights [host]: n positive finite numbers, used as they are (a caller wanting a mean passes weights that sum to 1).
 * rate in [0, 1]: rate 0 returns x.  With n = 1, scales = {1} and weights = {1} this is the last line of jat_bank_blend, bit
 * for bit.  y may be x; a track that overlaps y is refused (JAT_E_INVALID). */
int jat_bank_mix_scales(const float* x, int32_t n, const int32_t* scales, const float* const* tracks, const float* weights,
                        float rate, float* y, int32_t B, int32_t C, int32_t T, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* JAT_HIP_MS_H */
