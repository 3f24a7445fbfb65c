// DAC 44.1 kHz decoder kernels for gfx950 (HF transformers DacDecoder, modeling_dac.py:86-100,175-210,236-264,407-441).
//
// Layout: activations are channels-last, [rows = B * T', C] (token-major like the rest of csrc/).  Every convolution of the
// decoder is one implicit GEMM  out[m, n] = sum_{j < KT} sum_ci A[m + (j - (KT-1)/2) * dil, ci] * W[n, j, ci]:
//   - Conv1d k7, dilation d, padding 3d:      KT = 7, N = Cout;
//   - Conv1d k1 (residual unit conv2):        KT = 1, N = Cout, fp32 residual added in the epilogue;
//   - ConvTranspose1d k = 2s, stride s, pad s/2: polyphase, KT = 3 (dil 1), N = s * Cout.  Output o = q*s + r (phase r) reads
//     input frames q-1, q, q+1 with taps k = r + s/2 - shift*s (zero where k falls outside [0, 2s)); the [T, s, Cout] result is
//     already the interleaved [T*s, Cout] channels-last tensor.  Weights are laid out by the host (jat_dac.cpp: pack_weight).
// A row read outside [0, T') of its OWN sample is zero (checked per lane and tap), so batch rows never leak into each other.
// Operands are bf16 planes (hi, lo = bf16(v - hi)) of both activations and weights; precision "bf16x3" runs three MFMA passes
// (hi*hi + hi*lo + lo*hi) with fp32 accumulation, "bf16" one pass.  This file is independent of JAT_OPERAND_DTYPE: the fp16
// library computes the same bits.
// Epilogue: + bias, + fp32 residual, fp32 store (the residual stream), and the operand of the next conv as snake_{alpha}(v)
// (snake(x) = x + sin(alpha x)^2 / (alpha + 1e-9), modeling_dac.py:86-100) with sinf (full range reduction).
// Main loop: per 32-channel K chunk, the (BM + (KT-1)*dil) x 32 activation window and the BN x KT x 32 weight tile are staged
// in LDS once; all KT taps are formed from the window.  v_mfma_f32_16x16x32_bf16 with operands swapped (weight fragment as
// A) so each lane owns 4 consecutive output channels of one row: 16-B fp32 / 8-B operand stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jat_dac_kernels.h"

typedef __attribute__((ext_vector_type(8))) __bf16 dac_bf16x8;
typedef __attribute__((ext_vector_type(4))) float dac_f32x4;

namespace {

constexpr int BK = 32;   // channels per K chunk (one MFMA k-step)

__device__ __forceinline__ uint16_t f2bf(float f) { return __builtin_bit_cast(uint16_t, (__bf16)f); }
__device__ __forceinline__ float bf2f(uint16_t u) { return __builtin_bit_cast(float, (uint32_t)u << 16); }

__device__ __forceinline__ float snakef(float v, float a) {
  const float s = sinf(a * v);
  return v + (1.0f / (a + 1e-9f)) * (s * s);   // modeling_dac.py:98: x + (alpha + 1e-9).reciprocal() * sin(alpha x)^2
}

__device__ __forceinline__ void split_store4(uint16_t* hi, uint16_t* lo, int64_t off, const float (&s)[4]) {
  uint16_t h[4], l[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    h[k] = f2bf(s[k]);
    l[k] = f2bf(s[k] - bf2f(h[k]));
  }
  *(uint2*)(hi + off) = uint2{(uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16)};
  if (lo) *(uint2*)(lo + off) = uint2{(uint32_t)l[0] | ((uint32_t)l[1] << 16), (uint32_t)l[2] | ((uint32_t)l[3] << 16)};
}

// KT taps, HALO = (KT-1) * the largest dilation the instantiation serves; WM x WN waves of 32x32 (2x2 MFMA tiles) each.
template <int KT, int HALO, int WM, int WN, bool X3>
__global__ void __launch_bounds__(WM * WN * 64) dac_conv_kernel(const DacConvArgs p) {
  constexpr int BM = WM * 32, BN = WN * 32, NT = WM * WN * 64, PL = X3 ? 2 : 1, C = (KT - 1) / 2;
  constexpr int AROWS = BM + HALO;
  __shared__ __attribute__((aligned(16))) uint16_t sA[PL][AROWS][BK];
  __shared__ __attribute__((aligned(16))) uint16_t sW[PL][BN * KT][BK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int64_t m0 = (int64_t)blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const int arows = BM + (KT - 1) * p.dil;
  const int64_t g0 = m0 - (int64_t)C * p.dil;
  const uint16_t* ap[2] = {p.a_hi, p.a_lo};
  const uint16_t* wp[2] = {p.w_hi, p.w_lo};

  int tpos[2];   // position inside its own sample of the activation row this lane feeds (B operand column lane & 15)
#pragma unroll
  for (int ti = 0; ti < 2; ++ti) {
    const int64_t m = m0 + wm * 32 + ti * 16 + (lane & 15);
    tpos[ti] = m < p.M ? (int)(m % p.T) : -(1 << 30);
  }
  dac_f32x4 acc[2][2];
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int fi = 0; fi < 2; ++fi) acc[ti][fi] = dac_f32x4{0.f, 0.f, 0.f, 0.f};

  for (int c0 = 0; c0 < p.Cin; c0 += BK) {
    for (int idx = tid; idx < PL * arows * 4; idx += NT) {
      const int pl = idx / (arows * 4), rem = idx - pl * arows * 4, r = rem >> 2, q = rem & 3;
      const int64_t g = g0 + r;
      uint4 v = uint4{0u, 0u, 0u, 0u};
      if (g >= 0 && g < p.M) v = *(const uint4*)(ap[pl] + g * p.Cin + c0 + q * 8);
      *(uint4*)&sA[pl][r][(q ^ ((r >> 1) & 3)) * 8] = v;   // 16-B chunks XOR-swizzled by row pair
    }
    for (int idx = tid; idx < PL * BN * KT * 4; idx += NT) {
      const int pl = idx / (BN * KT * 4), rem = idx - pl * BN * KT * 4, r = rem >> 2, q = rem & 3;
      *(uint4*)&sW[pl][r][q * 8] = *(const uint4*)(wp[pl] + ((int64_t)n0 * KT + r) * p.Cin + c0 + q * 8);
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < KT; ++j) {
      dac_bf16x8 wf[PL][2], af[PL][2];
#pragma unroll
      for (int pl = 0; pl < PL; ++pl)
#pragma unroll
        for (int fi = 0; fi < 2; ++fi)
          wf[pl][fi] = *(const dac_bf16x8*)&sW[pl][(wn * 32 + fi * 16 + (lane & 15)) * KT + j][(lane >> 4) * 8];
#pragma unroll
      for (int ti = 0; ti < 2; ++ti) {
        const int r = wm * 32 + ti * 16 + (lane & 15) + j * p.dil;
        const bool ok = (unsigned)(tpos[ti] + (j - C) * p.dil) < (unsigned)p.T;
#pragma unroll
        for (int pl = 0; pl < PL; ++pl) {
          const dac_bf16x8 v = *(const dac_bf16x8*)&sA[pl][r][((lane >> 4) ^ ((r >> 1) & 3)) * 8];
          af[pl][ti] = ok ? v : dac_bf16x8{};
        }
      }
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int fi = 0; fi < 2; ++fi) {
          if constexpr (X3) {
            acc[ti][fi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[1][fi], af[0][ti], acc[ti][fi], 0, 0, 0);
            acc[ti][fi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[0][fi], af[1][ti], acc[ti][fi], 0, 0, 0);
          }
          acc[ti][fi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[0][fi], af[0][ti], acc[ti][fi], 0, 0, 0);
        }
    }
    __syncthreads();
  }

#pragma unroll
  for (int ti = 0; ti < 2; ++ti) {
    const int64_t m = m0 + wm * 32 + ti * 16 + (lane & 15);
    if (m >= p.M) continue;
#pragma unroll
    for (int fi = 0; fi < 2; ++fi) {
      const int n = n0 + wn * 32 + fi * 16 + 4 * (lane >> 4);
      const int c = n % p.Cch;
      const float4 b = *(const float4*)(p.bias + c);
      float v[4] = {acc[ti][fi][0] + b.x, acc[ti][fi][1] + b.y, acc[ti][fi][2] + b.z, acc[ti][fi][3] + b.w};
      const int64_t off = m * p.N + n;
      if (p.res) {
        const float4 r = *(const float4*)(p.res + off);
        v[0] = r.x + v[0], v[1] = r.y + v[1], v[2] = r.z + v[2], v[3] = r.w + v[3];   // modeling_dac.py:208
      }
      if (p.out32) *(float4*)(p.out32 + off) = float4{v[0], v[1], v[2], v[3]};
      if (p.o_hi) {
        const float4 a = *(const float4*)(p.alpha + c);
        const float s[4] = {snakef(v[0], a.x), snakef(v[1], a.y), snakef(v[2], a.z), snakef(v[3], a.w)};
        split_store4(p.o_hi, X3 ? p.o_lo : nullptr, off, s);
      }
    }
  }
}

// [B, C, T] fp32 latent -> channels-last operand planes [B*T, C] (32x32 tiles through LDS)
__global__ void __launch_bounds__(256) dac_z_split_kernel(const float* __restrict__ z, uint16_t* hi, uint16_t* lo, int C, int T) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z, c0 = blockIdx.y * 32, t0 = blockIdx.x * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) {
    const int t = t0 + tx;
    tile[i][tx] = t < T ? z[((int64_t)b * C + c0 + i) * T + t] : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int t = t0 + i;
    if (t >= T) continue;
    const float v = tile[tx][i];
    const int64_t off = ((int64_t)b * T + t) * C + c0 + tx;
    const uint16_t h = f2bf(v);
    hi[off] = h;
    if (lo) lo[off] = f2bf(v - bf2f(h));
  }
}

__global__ void dac_split_kernel(const float* __restrict__ x, uint16_t* hi, uint16_t* lo, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint16_t h = f2bf(x[i]);
    hi[i] = h;
    lo[i] = f2bf(x[i] - bf2f(h));
  }
}

// Tail (modeling_dac.py:436-439): snake -> Conv1d(C, 1, k7, p3) -> tanh.  N = 1 is not an MFMA shape: one thread per output
// sample, the snake of the (TILE + 6) x C fp32 window computed once into LDS.
constexpr int TAIL_TILE = 128, TAIL_CMAX = 96;
__global__ void __launch_bounds__(TAIL_TILE) dac_tail_kernel(const float* __restrict__ x, const float* __restrict__ alpha,
                                                             const float* __restrict__ w, const float* __restrict__ bias,
                                                             float* __restrict__ out, int C, int T, int64_t M) {
  __shared__ float sh[TAIL_TILE + 6][TAIL_CMAX + 1];
  const int64_t m0 = (int64_t)blockIdx.x * TAIL_TILE;
  for (int idx = threadIdx.x; idx < (TAIL_TILE + 6) * C; idx += TAIL_TILE) {
    const int r = idx / C, ci = idx - r * C;
    const int64_t g = m0 - 3 + r;
    sh[r][ci] = (g >= 0 && g < M) ? snakef(x[g * C + ci], alpha[ci]) : 0.f;
  }
  __syncthreads();
  const int64_t m = m0 + threadIdx.x;
  if (m >= M) return;
  const int t = (int)(m % T);
  float acc = bias[0];
  for (int k = 0; k < 7; ++k) {
    if ((unsigned)(t + k - 3) >= (unsigned)T) continue;   // padding = 3 of the sample's own edges
    const float* row = sh[threadIdx.x + k];
    for (int ci = 0; ci < C; ++ci) acc = __builtin_fmaf(w[k * C + ci], row[ci], acc);
  }
  out[m] = tanhf(acc);
}

template <int KT, int HALO, int WM, int WN>
hipError_t launch_conv_t(const DacConvArgs& p, bool x3, hipStream_t s) {
  const dim3 grid((unsigned)((p.M + WM * 32 - 1) / (WM * 32)), (unsigned)(p.N / (WN * 32)));
  if (x3) hipLaunchKernelGGL((dac_conv_kernel<KT, HALO, WM, WN, true>), grid, dim3(WM * WN * 64), 0, s, p);
  else hipLaunchKernelGGL((dac_conv_kernel<KT, HALO, WM, WN, false>), grid, dim3(WM * WN * 64), 0, s, p);
  return hipGetLastError();
}

template <int KT, int HALO>
hipError_t launch_conv_k(const DacConvArgs& p, bool x3, hipStream_t s) {
  // 64x64 tiles where N allows, else 128x32 (N = 96, 192 ... channel counts that are odd multiples of 32)
  return p.N % 64 == 0 ? launch_conv_t<KT, HALO, 2, 2>(p, x3, s) : launch_conv_t<KT, HALO, 4, 1>(p, x3, s);
}

}  // namespace

hipError_t dac_launch_conv(const DacConvArgs& p, int taps, bool x3, hipStream_t s) {
  if (p.M <= 0) return hipSuccess;
  switch (taps) {
    case 7: return launch_conv_k<7, 6 * DAC_MAX_DIL>(p, x3, s);
    case 3: return launch_conv_k<3, 2>(p, x3, s);
    case 1: return launch_conv_k<1, 0>(p, x3, s);
  }
  return hipErrorInvalidValue;
}

hipError_t dac_launch_z_split(const float* z, uint16_t* hi, uint16_t* lo, int B, int C, int T, hipStream_t s) {
  hipLaunchKernelGGL(dac_z_split_kernel, dim3((T + 31) / 32, C / 32, B), dim3(256), 0, s, z, hi, lo, C, T);
  return hipGetLastError();
}

hipError_t dac_launch_split(const float* x, uint16_t* hi, uint16_t* lo, int64_t n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int64_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(dac_split_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, x, hi, lo, n);
  return hipGetLastError();
}

hipError_t dac_launch_tail(const float* x, const float* alpha, const float* w, const float* bias, float* out, int C, int T,
                           int64_t M, hipStream_t s) {
  if (M <= 0) return hipSuccess;
  hipLaunchKernelGGL(dac_tail_kernel, dim3((unsigned)((M + TAIL_TILE - 1) / TAIL_TILE)), dim3(TAIL_TILE), 0, s, x, alpha, w,
                     bias, out, C, T, M);
  return hipGetLastError();
}
