// Launchers of the DAC decoder kernels (dac.hip), used by jat_dac.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int DAC_MAX_DIL = 9;   // largest dilation of a k7 residual-unit conv (modeling_dac.py:260-262: 1, 3, 9)

// out[m, n] = sum_j sum_ci A[m + (j - (taps-1)/2) * dil, ci] * W[n, j, ci] over rows of the same sample, then the epilogue.
struct DacConvArgs {
  const uint16_t *a_hi, *a_lo;   // [M, Cin] bf16 operand planes (a_lo unused in bf16 mode)
  const uint16_t *w_hi, *w_lo;   // [N, taps, Cin]
  const float* bias;             // [Cch], column n uses bias[n % Cch]
  const float* res;              // [M, N] fp32 residual added after the bias, or null
  float* out32;                  // [M, N] fp32 result, or null (may alias res)
  const float* alpha;            // [Cch] snake alpha of the next conv's operand (with o_hi)
  uint16_t *o_hi, *o_lo;         // [M, N] operand planes snake_alpha(result), or null
  int64_t M;                     // rows = B * T
  int T, Cin, N, Cch, dil;
};

hipError_t dac_launch_conv(const DacConvArgs& p, int taps, bool x3, hipStream_t s);
hipError_t dac_launch_z_split(const float* z, uint16_t* hi, uint16_t* lo, int B, int C, int T, hipStream_t s);
hipError_t dac_launch_split(const float* x, uint16_t* hi, uint16_t* lo, int64_t n, hipStream_t s);
hipError_t dac_launch_tail(const float* x, const float* alpha, const float* w, const float* bias, float* out, int C, int T,
                           int64_t M, hipStream_t s);

// Encoder (dac_enc.hip).  Head: conv1 = Conv1d(1, C, k7, pad 3) per sample on audio [B, L] (M = B * L rows); w torch
// [C, 1, 7]; out32 [M, C] fp32 and/or o_hi/o_lo [M, C] planes of snake_alpha(out) (o_lo may be null: bf16 only).
hipError_t dac_launch_head(const float* audio, const float* w, const float* bias, const float* alpha, float* out32,
                           uint16_t* o_hi, uint16_t* o_lo, int C, int L, int64_t M, hipStream_t s);

// Residual vector quantizer in fp32 (hidden size 1024, codebooks of 1024 x 8).
struct DacRvqArgs {
  const float* hidden;     // [M, 1024] channels-last (M = B * T)
  const float* w_in;       // [nq, 8, 1024] in_proj weights
  const float* b_in;       // [nq, 8]
  const float* codebook;   // [nq, 1024, 8] un-normalized (normalized in LDS by the kernel)
  const float* w_out;      // [nq, 1024, 8] out_proj weights
  const float* b_out;      // [nq, 1024]
  float* z;                // [B, 1024, T]
  int32_t* codes;          // [B, nq, T] or null
  float* latents;          // [B, 8 nq, T] in_proj outputs, or null
  float* hidden_cm;        // [B, 1024, T] copy of hidden, or null
  int64_t M;
  int T, nq;
};
hipError_t dac_launch_rvq(const DacRvqArgs& p, hipStream_t s);
