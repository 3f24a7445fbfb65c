// Multi-scale latent retrieval kernels for gfx950: the pooled bank pack, the one-launch pooling of the queries
// at every coarse scale, and the mix of the per-scale tracks back at the frame rate.  fp32 throughout, every operation rounded
// once (nothing fused but the mix's last line, below), so tests/retrieval_ms_ref.py restates them bit for bit.  The search, the norms and the per-scale blend
// are the kernels of retrieval.hip, unchanged.
//
// Pooling (bank rows and queries, one contract).  With q_j = (src_j - mean[c]) / std[c], the window of scale s that starts at
// frame f of a source of length len holds cnt = min(s, len - f) frames and pools to
//   p = (((q_f + q_{f+1}) + q_{f+2}) + ...) / float(cnt):  ascending sequential adds, then one division.
// s = 1 is q_f itself (q / 1.0f keeps every bit).
//
// Interpolation and mix.  The track v_i [B, C, Ts] of scale s, Ts = ceil(T / s), is read at frame t as
//   p = (t + 0.5) / s - 0.5, j0 = floor(p), w = p - j0, u = (1 - w) v[clamp(j0)] + w v[clamp(j0 + 1)]     (s = 1: u = v[t])
// in integers: 2 s p = 2 t + 1 - s, so j0 is an arithmetic shift and w a dyadic fraction, exact in fp32.  Then
//   m = -0; m = m + a_i u_i for i ascending;  y = fma(1 - r, x, r m).
// The last line is the one fused operation here: bank_blend_kernel's (1 - r) x + r v is compiled to v_mul (r v) and v_fmac, and
// a mix of scale 1 alone with weight 1 has to be that blend bit for bit, so the fma is written out.
// All three kernels stream: each input byte is read once from HBM (the mix's two taps of a track share lines between
// neighbouring lanes) and each output byte written once.
#include "jat_retrieval_kernels.h"

// One rounding per operation is the contract of this file.  The header's __fadd_rn / __fmul_rn are plain + and * compiled
// under the default contraction mode, and the backend does fuse such a product into the sum behind it (m + a u became one
// v_fmac_f32).  So contraction is switched off here and the operations are written through helpers defined under it.
#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ float add1(float a, float b) { return a + b; }
__device__ __forceinline__ float mul1(float a, float b) { return a * b; }
__device__ __forceinline__ float div1(float a, float b) { return a / b; }   // correctly rounded (hipcc's default for fp32 /)

__device__ __forceinline__ uint16_t f2h(float f) { return __builtin_bit_cast(uint16_t, (_Float16)f); }

// ---- pooled pack: bank_pack_kernel with the window loop ---------------------------------------------------------------------
// 32 windows x 32 channels per block through LDS: lanes along the windows on the read, along the channels on the write.
template <typename S>
__global__ __launch_bounds__(RT_THREADS) void bank_pack_pool_kernel(const S* __restrict__ src, const S* __restrict__ src2,
                                                                    int64_t len, int64_t first, int64_t stride, int count,
                                                                    int window, const float* __restrict__ mean,
                                                                    const float* __restrict__ sd,
                                                                    const float* __restrict__ mean2,
                                                                    const float* __restrict__ sd2, uint16_t* __restrict__ rows,
                                                                    uint16_t* __restrict__ rows2, int64_t row0, int C) {
  __shared__ float tile[32][33];
  const int second = blockIdx.z;
  const S* in = second ? src2 : src;
  const float* mu = second ? mean2 : mean;
  const float* sg = second ? sd2 : sd;
  uint16_t* out = second ? rows2 : rows;
  const int f0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int lo = threadIdx.x & 31, hi = threadIdx.x >> 5;
  const int i = f0 + lo;
  if (i < count) {
    const int64_t frame = first + (int64_t)i * stride;                 // < len: checked by the caller
    const int64_t left = len - frame;
    const int cnt = left < window ? (int)left : window;                // the window is cut by the end of the source
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = c0 + hi + 8 * k;
      const S* p = in + (int64_t)c * len + frame;
      const float m = mu[c], s = sg[c];
      float acc = ((float)p[0] - m) / s;                               // the expression of channel_affine_kernel
      for (int j = 1; j < cnt; ++j) acc = add1(acc, ((float)p[j] - m) / s);
      tile[hi + 8 * k][lo] = div1(acc, (float)cnt);
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int j = f0 + hi + 8 * k;
    if (j < count) out[(row0 + j) * C + c0 + lo] = f2h(tile[lo][hi + 8 * k]);
  }
}

// ---- pooled queries: x [B, C, T] read once, every requested scale written ---------------------------------------------------
// A block owns 32 channels x RT_POOL_FRAMES frames.  Read: the 256 threads take 256 consecutive frames of one channel per step
// (full 128-byte lines).  A frame t of the tile sits at LDS word t + t / 32: one pad word per 32 frames, so the read of the
// window sums, lanes s words apart, touches every bank once per 32 lanes for s = 2, 4 and 8 (lane l reads word
// l s + k + (l s + k) / 32; the lanes whose l s falls into the same 32-frame group are s banks apart, and each further group is
// shifted by one bank).  Write: lanes along ts.  The tile starts at a multiple of 8, so no window crosses a tile.
constexpr int POOL_ROW = RT_POOL_FRAMES + RT_POOL_FRAMES / 32;   // words per channel row of the tile

template <bool NORM>
__global__ __launch_bounds__(RT_THREADS) void bank_pool_queries_kernel(const float* __restrict__ x,
                                                                       const float* __restrict__ mean,
                                                                       const float* __restrict__ sd, int C, int T,
                                                                       RtPoolArgs a) {
  __shared__ float tile[32][POOL_ROW];
  const int t0 = blockIdx.x * RT_POOL_FRAMES, c0 = blockIdx.y * 32, b = blockIdx.z;
  const int tid = threadIdx.x;
  const int live = min(RT_POOL_FRAMES, T - t0);                        // frames of this tile inside the source
  const float* xp = x + ((int64_t)b * C + c0) * T + t0 + tid;
  if (tid < live) {
    const int w = tid + (tid >> 5);
#pragma unroll 8
    for (int c = 0; c < 32; ++c) {
      const float v = xp[(int64_t)c * T];
      tile[c][w] = NORM ? (v - mean[c0 + c]) / sd[c0 + c] : v;         // the expression of channel_affine_kernel
    }
  }
  __syncthreads();
  for (int i = 0; i < a.n; ++i) {
    const int s = a.scale[i], sh = 31 - __clz(s);                      // s in {2, 4, 8}
    const int Ts = (T + s - 1) >> sh;                                  // pooled frames of the whole source
    const int per = RT_POOL_FRAMES >> sh;                              // pooled frames of a full tile
    const int have = (live + s - 1) >> sh;                             // pooled frames of this tile
    float* out = a.out[i] + ((int64_t)b * C + c0) * Ts + (t0 >> sh);
    for (int e = tid; e < 32 * per; e += RT_THREADS) {
      const int c = e >> (8 - sh), j = e & (per - 1);                  // per = 2^(8 - sh)
      if (j >= have) continue;
      const int f = j << sh;
      const int cnt = min(s, live - f);
      float acc = tile[c][f + (f >> 5)];
      for (int k = 1; k < cnt; ++k) acc = add1(acc, tile[c][f + k + ((f + k) >> 5)]);
      out[(int64_t)c * Ts + j] = div1(acc, (float)cnt);
    }
  }
}

// ---- mix: y = (1 - r) x + r sum_i a_i interp(v_i) ---------------------------------------------------------------------------
// Lanes along t; a block row walks the (b, c) rows.  x and y are not restrict: y may be x.
__global__ __launch_bounds__(RT_THREADS) void bank_mix_scales_kernel(const float* x, RtMixArgs a, float rate, float* y,
                                                                     int64_t rows, int T) {
  const int t = blockIdx.x * RT_THREADS + threadIdx.x;
  if (t >= T) return;
  const float keep = 1.f - rate;
  // the taps of frame t at every scale: the same for all rows
  int ja[RT_MAX_SCALES], jb[RT_MAX_SCALES], Ts[RT_MAX_SCALES];
  float w[RT_MAX_SCALES];
#pragma unroll
  for (int i = 0; i < RT_MAX_SCALES; ++i) {
    ja[i] = jb[i] = t, Ts[i] = T, w[i] = 0.f;
    if (i < a.n && a.scale[i] > 1) {
      const int s = a.scale[i], sh = 31 - __clz(s);
      Ts[i] = (T + s - 1) >> sh;
      const int num = 2 * t + 1 - s;                                   // 2 s p; may be negative
      const int j0 = num >> (sh + 1);                                  // floor(p): an arithmetic shift
      w[i] = ldexpf((float)(num - j0 * 2 * s), -(sh + 1));               // p - j0 = remainder / 2 s: a dyadic fraction, exact
      ja[i] = min(max(j0, 0), Ts[i] - 1);
      jb[i] = min(max(j0 + 1, 0), Ts[i] - 1);
    }
  }
  for (int64_t row = blockIdx.y; row < rows; row += gridDim.y) {
    float m = -0.f;
#pragma unroll
    for (int i = 0; i < RT_MAX_SCALES; ++i) {
      if (i < a.n) {
        const float* v = a.v[i] + row * Ts[i];
        float u;
        if (a.scale[i] == 1)
          u = v[t];
        else
          u = add1(mul1(1.f - w[i], v[ja[i]]), mul1(w[i], v[jb[i]]));
        m = add1(m, mul1(a.a[i], u));
      }
    }
    const int64_t off = row * T + t;
    y[off] = fmaf(keep, x[off], mul1(rate, m));       // what bank_blend_kernel's last line compiles to: r m rounded, one fma
  }
}

}  // namespace

hipError_t bank_pack_pool_launch(const void* src, const void* src2, bool src_fp16, int64_t len, int64_t first, int64_t stride,
                                 int count, int window, const float* mean, const float* std, const float* mean2,
                                 const float* std2, uint16_t* rows, uint16_t* rows2, int64_t row0, int C, hipStream_t s) {
  if (count <= 0) return hipSuccess;
  const dim3 grid((unsigned)((count + 31) / 32), (unsigned)(C / 32), src2 ? 2u : 1u), block(RT_THREADS);
  if (src_fp16)
    hipLaunchKernelGGL(bank_pack_pool_kernel<_Float16>, grid, block, 0, s, (const _Float16*)src, (const _Float16*)src2, len,
                       first, stride, count, window, mean, std, mean2, std2, rows, rows2, row0, C);
  else
    hipLaunchKernelGGL(bank_pack_pool_kernel<float>, grid, block, 0, s, (const float*)src, (const float*)src2, len, first,
                       stride, count, window, mean, std, mean2, std2, rows, rows2, row0, C);
  return hipGetLastError();
}

hipError_t bank_pool_queries_launch(const float* x, const float* mean, const float* std, int B, int C, int T,
                                    const RtPoolArgs& a, hipStream_t s) {
  static_assert(RT_POOL_FRAMES == RT_THREADS && RT_POOL_FRAMES % 32 == 0, "one frame of the tile per thread on the read");
  if (a.n <= 0) return hipSuccess;
  const dim3 grid((unsigned)((T + RT_POOL_FRAMES - 1) / RT_POOL_FRAMES), (unsigned)(C / 32), (unsigned)B), block(RT_THREADS);
  if (mean)
    hipLaunchKernelGGL(bank_pool_queries_kernel<true>, grid, block, 0, s, x, mean, std, C, T, a);
  else
    hipLaunchKernelGGL(bank_pool_queries_kernel<false>, grid, block, 0, s, x, mean, std, C, T, a);
  return hipGetLastError();
}

hipError_t bank_mix_scales_launch(const float* x, const RtMixArgs& a, float rate, float* y, int B, int C, int T,
                                  hipStream_t s) {
  const int64_t rows = (int64_t)B * C;
  const dim3 grid((unsigned)((T + RT_THREADS - 1) / RT_THREADS), (unsigned)(rows < 65535 ? rows : 65535)), block(RT_THREADS);
  hipLaunchKernelGGL(bank_mix_scales_kernel, grid, block, 0, s, x, a, rate, y, rows, T);
  return hipGetLastError();
}
