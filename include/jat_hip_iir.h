/*
 * jat_hip_iir.h — C ABI of the IIR low-pass cascades, an addition to jat_hip.h: scipy's `sosfilt` and
 * `sosfiltfilt` (default padding) for batches of rows, each row with a filter of its own out of a table of R filters, computed
 * as an exact blocked linear recurrence by csrc/iir.hip.  The conventions of jat_hip.h hold: device pointers unless marked
 * [host], fp32 in both operand-dtype builds, every filtering call only enqueues on the caller's stream, none of them
 * synchronises, allocates or copies, and each may be captured into a graph.  A refused call returns JAT_E_INVALID (JAT_E_STATE
 * for a workspace that is too small), launches nothing and writes nothing.  No kernel uses atomics and no workgroup waits for
 * another: the bits repeat from run to run and do not depend on B.
 *
 * Definitions
 *   Filter.  JAT_IIR_SECTIONS = 5 second-order sections in scipy's layout {b0, b1, b2, a0, a1, a2} with a0 = 1.  A shorter
 *     cascade is padded BEHIND its own sections with identity sections {1, 0, 0, 1, 0, 0}; S is the number of sections up to
 *     the last one that is not an identity.  Identity padding is skipped, not multiplied through: a filter of S = 0 returns x.
 *   Section (direct form II transposed, scipy's):  y = b0 x + s1;  s1 = (b1 x - a1 y) + s2;  s2 = b2 x - a2 y, every product
 *     and sum rounded once to fp32 (nothing is fused), sections in order, the output of one the input of the next.
 *   padlen = 3 (2 S + 1 - min(#sections with b2 = 0, #sections with a2 = 0)) over the filter's own S sections: scipy's default.
 *   jat_iir_sosfilt: the cascade over x[0 .. n) from zero state.
 *   jat_iir_sosfiltfilt: x_ext = the odd extension of x by padlen samples on each side (2 x[0] - x[padlen - i] in front,
 *     2 x[n-1] - x[n-2-i] behind, read through an index map, never copied); a forward pass over x_ext from state
 *     zi * x_ext[0]; a backward pass over that result from state zi * (its last sample); the extension dropped.
 *   Blocking.  A lane owns lane_block consecutive samples and a workgroup a tile (jat_iir_geometry).  The state behind a block
 *     that started from state s is P s + e with P = A^lane_block, A the zero-input transition of the whole cascade in its 10
 *     state coordinates {s1, s2} x 5 and e the state behind the block run from zero.  powers[k] = P^(2^k), k = 0 .. 8, so
 *     powers[8] = A^tile.  Pass A runs every block from zero and scans the maps inside each tile (step k: e[l] = e[l] +
 *     powers[k] e[l - 2^k], the sum taken in the order e + m0 v0 + m1 v1 + ...), pass B carries the tile states along the row
 *     with powers[8], pass C repeats the scan from each tile's true start state and re-runs every block from its true start
 *     state on the real input.  Within a block the arithmetic is the sequential recurrence's; tests/lowpass_ref.py states all of
 *     it in numpy with the same rounding points.
 *   The device cannot refuse a row_filter entry outside 0 .. R-1 without waiting for it: the kernels clamp it into range (no wild
 *     read), and the Python binding checks the indices on the host before it uploads them.
 */
#ifndef JAT_HIP_IIR_H
#define JAT_HIP_IIR_H

#include "jat_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define JAT_IIR_SECTIONS 5
#define JAT_IIR_POWERS 9
#define JAT_IIR_MAX_PADLEN 33
#define JAT_IIR_MAX_FILTERS 4096
#define JAT_IIR_MAX_N (1 << 30)

/* [host] sos fp64 [R, 5, 6], zi fp64 [R, 5, 2] (scipy's sosfilt_zi; zero for identity sections), powers fp64 [R, 9, 10, 10]
 * (above) -> a handle holding the fp32 tables on the device.  Allocates, copies and waits for `stream`.  JAT_E_INVALID: a null
 * pointer, R outside 1..4096, a value that is not finite, a0 != 1, a section that is not an identity behind an identity. */
int jat_iir_create(const double* sos, const double* zi, const double* powers, int32_t R, void* stream, void** handle);
void jat_iir_destroy(void* handle);

/* samples per lane and per workgroup; either pointer may be NULL */
int jat_iir_geometry(int32_t* lane_block, int32_t* tile);
/* the largest padlen of the handle's filters: jat_iir_sosfiltfilt refuses n <= this, for every row of the call */
int jat_iir_padlen(const void* handle, int32_t* padlen);
/* bytes of the caller-owned workspace for [B, n] (either call); JAT_E_INVALID: B outside 1..65535, n outside 1..2^30 */
int jat_iir_workspace_bytes(int32_t B, int64_t n, size_t* bytes);

/* x fp32 [B, n], row_filter int32 [B] (device) -> y fp32 [B, n]; y may be x (any other overlap is the caller's error).
 * JAT_E_INVALID: a null handle or buffer, B outside 1..65535, n outside 1..2^30.  JAT_E_STATE: workspace_bytes too small. */
int jat_iir_sosfilt(void* handle, const int32_t* row_filter, const float* x, float* y, int32_t B, int64_t n, void* workspace,
                    size_t workspace_bytes, void* stream);
/* the same arguments; also JAT_E_INVALID for n <= jat_iir_padlen(handle), as scipy refuses it */
int jat_iir_sosfiltfilt(void* handle, const int32_t* row_filter, const float* x, float* y, int32_t B, int64_t n, void* workspace,
                        size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* JAT_HIP_IIR_H */
