// DAC 44.1 kHz encoder kernels for gfx950 (HF transformers DacEncoder + DacResidualVectorQuantizer, modeling_dac.py:103-173,
// 212-234, 283-345, 444-475).  The residual units, the strided down-sampling convs and conv2 run on dac_conv_kernel
// (dac.hip); this file holds the two stages that are not MFMA shapes:
//   - head: conv1 = Conv1d(1, C, k7, pad 3) on the audio, VALU, with the decoder's epilogue roles (fp32 stream + snake planes);
//   - RVQ: the residual vector quantizer in fp32, every codebook of a frame in one workgroup (the codebook loop is
//     sequential per frame).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "jat_dac_kernels.h"

namespace {

// The same roundings as dac.hip's epilogue (bf16 round-to-nearest-even planes, snake with sinf), so the encoder's operand
// planes are formed exactly as the convs' own epilogue forms them.
__device__ __forceinline__ uint16_t f2bf(float f) { return __builtin_bit_cast(uint16_t, (__bf16)f); }
__device__ __forceinline__ float bf2f(uint16_t u) { return __builtin_bit_cast(float, (uint32_t)u << 16); }

__device__ __forceinline__ float snakef(float v, float a) {
  const float s = sinf(a * v);
  return v + (1.0f / (a + 1e-9f)) * (s * s);   // modeling_dac.py:98
}

// conv1 (modeling_dac.py:450): one thread per (row, 4 output channels), the 7 taps read from the sample's own audio
// (zero outside [0, L) of that sample).  w is torch's [C, 1, 7].
__global__ void __launch_bounds__(256) dac_head_kernel(const float* __restrict__ audio, const float* __restrict__ w,
                                                       const float* __restrict__ bias, const float* __restrict__ alpha,
                                                       float* out32, uint16_t* o_hi, uint16_t* o_lo, int C, int L,
                                                       int64_t M) {
  const int cq = C >> 2;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t m = idx / cq;
  if (m >= M) return;
  const int c = (int)(idx - m * cq) * 4, t = (int)(m % L);
  float x[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) x[k] = (unsigned)(t + k - 3) < (unsigned)L ? audio[m + k - 3] : 0.f;
  float v[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    float acc = bias[c + u];
#pragma unroll
    for (int k = 0; k < 7; ++k) acc = __builtin_fmaf(w[(c + u) * 7 + k], x[k], acc);
    v[u] = acc;
  }
  const int64_t off = m * C + c;
  if (out32) *(float4*)(out32 + off) = float4{v[0], v[1], v[2], v[3]};
  if (o_hi) {
    uint16_t h[4], l[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float s = snakef(v[u], alpha[c + u]);
      h[u] = f2bf(s);
      l[u] = f2bf(s - bf2f(h[u]));
    }
    *(uint2*)(o_hi + off) = uint2{(uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16)};
    if (o_lo) *(uint2*)(o_lo + off) = uint2{(uint32_t)l[0] | ((uint32_t)l[1] << 16), (uint32_t)l[2] | ((uint32_t)l[3] << 16)};
  }
}

// F.normalize of an 8-vector (x / max(||x||, 1e-12)), one fixed fp32 order for codewords and projected latents alike.
__device__ __forceinline__ void normalize8(float (&v)[8]) {
  float ss = v[0] * v[0];
#pragma unroll
  for (int k = 1; k < 8; ++k) ss = __builtin_fmaf(v[k], v[k], ss);
  const float d = fmaxf(sqrtf(ss), 1e-12f);
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = v[k] / d;
}

// RVQ (modeling_dac.py:283-345 in eval mode, DacVectorQuantize :103-173).  A workgroup of RVQ_WAVES waves owns
// RVQ_WAVES * RVQ_FPW consecutive frames; lane l of a wave holds channels q*256 + 4l + {0..3} (q < 4) of its frames'
// residual and z in registers through all codebooks.  Per codebook i:
//   stage normalize(codebook_i) in LDS (32 KB) -> e = in_proj_i(r) (per-lane partial dot products + xor butterfly, so every
//   lane holds the same bits) -> argmax over the 1024 normalized codewords (lane l scores j = 64w + l, strict > keeps the
//   lowest index, the butterfly prefers the lower index on equal scores) -> q = out_proj_i(codebook_i[idx]) (un-normalized
//   row) -> z += q, r -= q.
constexpr int RVQ_H = 1024, RVQ_CD = 8, RVQ_NC = 1024, RVQ_WAVES = 4, RVQ_FPW = 4, RVQ_FR = RVQ_WAVES * RVQ_FPW;

__global__ void __launch_bounds__(RVQ_WAVES * 64) dac_rvq_kernel(const DacRvqArgs p) {
  __shared__ float4 scb[RVQ_NC * 2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int64_t row[RVQ_FPW];
  int bb[RVQ_FPW], tt[RVQ_FPW];
  bool ok[RVQ_FPW];
  float r[RVQ_FPW][16], z[RVQ_FPW][16];
#pragma unroll
  for (int f = 0; f < RVQ_FPW; ++f) {
    row[f] = (int64_t)blockIdx.x * RVQ_FR + wave * RVQ_FPW + f;
    ok[f] = row[f] < p.M;
    bb[f] = ok[f] ? (int)(row[f] / p.T) : 0;
    tt[f] = ok[f] ? (int)(row[f] % p.T) : 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = q * 256 + lane * 4;
      float4 v = float4{0.f, 0.f, 0.f, 0.f};
      if (ok[f]) v = *(const float4*)(p.hidden + row[f] * RVQ_H + c);
      r[f][q * 4 + 0] = v.x, r[f][q * 4 + 1] = v.y, r[f][q * 4 + 2] = v.z, r[f][q * 4 + 3] = v.w;
      if (ok[f] && p.hidden_cm)
#pragma unroll
        for (int u = 0; u < 4; ++u) p.hidden_cm[((int64_t)bb[f] * RVQ_H + c + u) * p.T + tt[f]] = r[f][q * 4 + u];
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) z[f][u] = 0.f;
  }

  for (int i = 0; i < p.nq; ++i) {
    const float* cb = p.codebook + (int64_t)i * RVQ_NC * RVQ_CD;
    __syncthreads();   // the previous codebook's readers are done
    for (int j = tid; j < RVQ_NC; j += RVQ_WAVES * 64) {
      float v[8];
      const float4 a = *(const float4*)(cb + j * 8), b = *(const float4*)(cb + j * 8 + 4);
      v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
      normalize8(v);
      scb[2 * j] = float4{v[0], v[1], v[2], v[3]};
      scb[2 * j + 1] = float4{v[4], v[5], v[6], v[7]};
    }
    __syncthreads();

    // e = in_proj_i(r): W [8, 1024] (the 1x1 conv's [8, 1024, 1]), bias [8]
    float e[RVQ_FPW][RVQ_CD];
#pragma unroll
    for (int k = 0; k < RVQ_CD; ++k) {
#pragma unroll
      for (int f = 0; f < RVQ_FPW; ++f) e[f][k] = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 w = *(const float4*)(p.w_in + ((int64_t)i * RVQ_CD + k) * RVQ_H + q * 256 + lane * 4);
#pragma unroll
        for (int f = 0; f < RVQ_FPW; ++f) {
          e[f][k] = __builtin_fmaf(w.x, r[f][q * 4 + 0], e[f][k]);
          e[f][k] = __builtin_fmaf(w.y, r[f][q * 4 + 1], e[f][k]);
          e[f][k] = __builtin_fmaf(w.z, r[f][q * 4 + 2], e[f][k]);
          e[f][k] = __builtin_fmaf(w.w, r[f][q * 4 + 3], e[f][k]);
        }
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
      for (int f = 0; f < RVQ_FPW; ++f)
#pragma unroll
        for (int k = 0; k < RVQ_CD; ++k) e[f][k] += __shfl_xor(e[f][k], off);
#pragma unroll
    for (int f = 0; f < RVQ_FPW; ++f)
#pragma unroll
      for (int k = 0; k < RVQ_CD; ++k) e[f][k] += p.b_in[i * RVQ_CD + k];
    if (p.latents && lane == 0)
#pragma unroll
      for (int f = 0; f < RVQ_FPW; ++f)
        if (ok[f])
#pragma unroll
          for (int k = 0; k < RVQ_CD; ++k)
            p.latents[((int64_t)bb[f] * p.nq * RVQ_CD + i * RVQ_CD + k) * p.T + tt[f]] = e[f][k];

    // argmax_j <normalize(e), normalize(c_j)>
    float best[RVQ_FPW];
    int bi[RVQ_FPW];
#pragma unroll
    for (int f = 0; f < RVQ_FPW; ++f) {
      normalize8(e[f]);
      best[f] = -INFINITY;
      bi[f] = lane;
    }
    for (int w = 0; w < RVQ_NC / 64; ++w) {
      const int j = w * 64 + lane;
      const float4 c0 = scb[2 * j], c1 = scb[2 * j + 1];
#pragma unroll
      for (int f = 0; f < RVQ_FPW; ++f) {
        float s = e[f][0] * c0.x;
        s = __builtin_fmaf(e[f][1], c0.y, s);
        s = __builtin_fmaf(e[f][2], c0.z, s);
        s = __builtin_fmaf(e[f][3], c0.w, s);
        s = __builtin_fmaf(e[f][4], c1.x, s);
        s = __builtin_fmaf(e[f][5], c1.y, s);
        s = __builtin_fmaf(e[f][6], c1.z, s);
        s = __builtin_fmaf(e[f][7], c1.w, s);
        if (s > best[f]) best[f] = s, bi[f] = j;
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
      for (int f = 0; f < RVQ_FPW; ++f) {
        const float ob = __shfl_xor(best[f], off);
        const int oi = __shfl_xor(bi[f], off);
        if (ob > best[f] || (ob == best[f] && oi < bi[f])) best[f] = ob, bi[f] = oi;
      }
    if (p.codes && lane == 0)
#pragma unroll
      for (int f = 0; f < RVQ_FPW; ++f)
        if (ok[f]) p.codes[((int64_t)bb[f] * p.nq + i) * p.T + tt[f]] = bi[f];

    // q = out_proj_i(codebook_i[idx]): W [1024, 8] (the 1x1 conv's [1024, 8, 1]), bias [1024]
    float cv[RVQ_FPW][RVQ_CD];
#pragma unroll
    for (int f = 0; f < RVQ_FPW; ++f) {
      const float4 a = *(const float4*)(cb + bi[f] * 8), b = *(const float4*)(cb + bi[f] * 8 + 4);
      cv[f][0] = a.x, cv[f][1] = a.y, cv[f][2] = a.z, cv[f][3] = a.w, cv[f][4] = b.x, cv[f][5] = b.y, cv[f][6] = b.z, cv[f][7] = b.w;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int c = q * 256 + lane * 4 + u;
        const float* wr = p.w_out + ((int64_t)i * RVQ_H + c) * RVQ_CD;
        const float4 wa = *(const float4*)wr, wb = *(const float4*)(wr + 4);
        const float bo = p.b_out[i * RVQ_H + c];
#pragma unroll
        for (int f = 0; f < RVQ_FPW; ++f) {
          float v = bo;
          v = __builtin_fmaf(wa.x, cv[f][0], v);
          v = __builtin_fmaf(wa.y, cv[f][1], v);
          v = __builtin_fmaf(wa.z, cv[f][2], v);
          v = __builtin_fmaf(wa.w, cv[f][3], v);
          v = __builtin_fmaf(wb.x, cv[f][4], v);
          v = __builtin_fmaf(wb.y, cv[f][5], v);
          v = __builtin_fmaf(wb.z, cv[f][6], v);
          v = __builtin_fmaf(wb.w, cv[f][7], v);
          z[f][q * 4 + u] += v;   // modeling_dac.py:331-332
          r[f][q * 4 + u] -= v;
        }
      }
  }

#pragma unroll
  for (int f = 0; f < RVQ_FPW; ++f) {
    if (!ok[f]) continue;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int u = 0; u < 4; ++u) p.z[((int64_t)bb[f] * RVQ_H + q * 256 + lane * 4 + u) * p.T + tt[f]] = z[f][q * 4 + u];
  }
}

}  // namespace

hipError_t dac_launch_head(const float* audio, const float* w, const float* bias, const float* alpha, float* out32,
                           uint16_t* o_hi, uint16_t* o_lo, int C, int L, int64_t M, hipStream_t s) {
  if (M <= 0) return hipSuccess;
  const int64_t threads = M * (C / 4);
  hipLaunchKernelGGL(dac_head_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, audio, w, bias, alpha, out32,
                     o_hi, o_lo, C, L, M);
  return hipGetLastError();
}

hipError_t dac_launch_rvq(const DacRvqArgs& p, hipStream_t s) {
  if (p.M <= 0) return hipSuccess;
  hipLaunchKernelGGL(dac_rvq_kernel, dim3((unsigned)((p.M + RVQ_FR - 1) / RVQ_FR)), dim3(RVQ_WAVES * 64), 0, s, p);
  return hipGetLastError();
}
