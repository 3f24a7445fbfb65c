// Training-data kernels: batch assembly from the fp16 latent store and the per-step monitor sums.  fp32 / fp64 in both
// operand-dtype builds.
#include "jat_data_kernels.h"

namespace {

__device__ __forceinline__ float half_bits_to_float(unsigned short h) { return (float)__builtin_bit_cast(_Float16, h); }

// ---- crop + fp16 -> fp32 + per-channel normalisation (train_ddp_v3mod2.py:517-533, 856-857) ------------------------
// One wave per output row (tensor, b, c).  A source row starts at byte 2 (c len + start): 2-byte aligned only.  The wave
// copies the 16-byte-aligned span that covers the crop into its LDS row with 16-byte loads, then every lane picks the halves
// of its output vector at the shifted offset and stores V floats at once: V = 4 when T % 4 == 0 (every row start is
// 16-byte aligned), else V = 2 with one scalar float ahead of the vectors on rows that start on an odd element and one
// behind them where a single element is left.  Clips shorter than T (or a start that would run past the end) take the
// element-wise path with the index (start + j) mod len: the loop-repeat of :520-524.
template <int V>
__global__ __launch_bounds__(DT_THREADS) void latent_gather_kernel(
    const void* const* __restrict__ hr_src, const void* const* __restrict__ lr_src, const int64_t* __restrict__ len_t,
    const int64_t* __restrict__ start_t, const float* __restrict__ hr_mean, const float* __restrict__ hr_std,
    const float* __restrict__ lr_mean, const float* __restrict__ lr_std, float* __restrict__ hr_out,
    float* __restrict__ lr_out, int B, int C, int T, int row_halves) {
  extern __shared__ uint4 lds4[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t rows = (int64_t)B * C;
  const int64_t r2 = (int64_t)blockIdx.x * DT_ROWS + wave;
  unsigned short* row = (unsigned short*)lds4 + (size_t)wave * row_halves;
  int which = 0, c = 0, head = 0;
  int64_t r = 0;
  bool live = r2 < 2 * rows;
  if (live) {
    which = r2 >= rows;
    r = r2 - (which ? rows : 0);
    const int b = (int)(r / C);
    c = (int)(r - (int64_t)b * C);
    const int64_t len = len_t[b], st = start_t[b];
    const unsigned short* base = (const unsigned short*)(which ? lr_src[b] : hr_src[b]);
    if (len < 1 || base == nullptr) {
      live = false;                          // a malformed table entry: the row is left as it was
    } else if (st >= 0 && st + T <= len) {
      const uintptr_t a = (uintptr_t)(base + (int64_t)c * len + st);
      head = (int)((a & 15) >> 1);
      const uint4* a0 = (const uint4*)(a & ~(uintptr_t)15);
      const int nch = (head + T + 7) >> 3;   // <= row_halves / 8
      uint4* row4 = (uint4*)row;
      for (int k0 = lane; k0 < nch; k0 += 256) {   // four loads in flight per lane; a clamped index re-reads the last chunk
        const int k1 = k0 + 64, k2 = k0 + 128, k3 = k0 + 192, last = nch - 1;
        const uint4 v0 = a0[k0], v1 = a0[k1 < last ? k1 : last], v2 = a0[k2 < last ? k2 : last], v3 = a0[k3 < last ? k3 : last];
        row4[k0] = v0;
        if (k1 < nch) row4[k1] = v1;
        if (k2 < nch) row4[k2] = v2;
        if (k3 < nch) row4[k3] = v3;
      }
    } else {
      const unsigned short* rb = base + (int64_t)c * len;
      const int64_t m = ((st % len) + len) % len;
      for (int j = lane; j < T; j += 64) row[j] = rb[(m + j) % len];
    }
  }
  __syncthreads();   // a wave-level ordering instead (each wave reads back only its own row) measured the same: 113.0 vs 111.9 us
  if (!live) return;
  const float* mean = which ? lr_mean : hr_mean;
  const float* sd = which ? lr_std : hr_std;
  const bool norm = mean != nullptr;
  const float mu = norm ? mean[c] : 0.f, sg = norm ? sd[c] : 1.f;
  float* o = (which ? lr_out : hr_out) + r * T;
  const unsigned short* x = row + head;
  auto cv = [&](int j) {
    const float f = half_bits_to_float(x[j]);
    return norm ? (f - mu) / sg : f;         // the expression of channel_affine_kernel
  };
  const int hd = V == 4 ? 0 : (int)((r * T) & 1);
  const int nvec = (T - hd) / V;
  if (hd && lane == 0) o[0] = cv(0);
  for (int i = lane; i < nvec; i += 64) {
    const int j = hd + i * V;
    if (V == 4) {
      float4 v;
      v.x = cv(j), v.y = cv(j + 1), v.z = cv(j + 2), v.w = cv(j + 3);
      *(float4*)(o + j) = v;
    } else {
      float2 v;
      v.x = cv(j), v.y = cv(j + 1);
      *(float2*)(o + j) = v;
    }
  }
  if (hd + nvec * V < T && lane == 63) o[T - 1] = cv(T - 1);   // V == 2 only: at most one element is left
}

// ---- per-step monitor sums (train_ddp_v3mod2.py:902-919) ----------------------------------------------------------
// sums: 0 sum p, 1 sum p^2, 2 sum h^2, 3 sum (p - h)^2, 4 sum l, 5 sum l^2; every term formed and added in fp64
struct Mon {
  double a[MON_SUMS];
};
__device__ __forceinline__ void mon_add(Mon& m, float pf, float hf) {
  const double p = pf, h = hf, d = p - h;
  m.a[0] += p, m.a[1] += p * p, m.a[2] += h * h, m.a[3] += d * d;
}
__device__ __forceinline__ void mon_add_cond(Mon& m, float lf) {
  const double l = lf;
  m.a[4] += l, m.a[5] += l * l;
}
// lanes, then waves, in a fixed order; the block's sums end in thread 0
__device__ __forceinline__ void mon_block_reduce(Mon& m, double (*sh)[MON_SUMS]) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int q = 0; q < MON_SUMS; ++q) {
    double v = m.a[q];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) sh[wave][q] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < MON_SUMS; ++q) {
      double v = sh[0][q];
      for (int w = 1; w < MON_THREADS / 64; ++w) v += sh[w][q];
      m.a[q] = v;
    }
  }
}

__global__ __launch_bounds__(MON_THREADS) void train_monitor_partial_kernel(const float* __restrict__ pred,
                                                                            const float* __restrict__ target,
                                                                            const float* __restrict__ cond, int64_t n,
                                                                            double* __restrict__ partial) {
  __shared__ double sh[MON_THREADS / 64][MON_SUMS];
  Mon m = {};
  const int64_t gid = (int64_t)blockIdx.x * MON_THREADS + threadIdx.x, stride = (int64_t)MON_BLOCKS * MON_THREADS;
  const int64_t nv = n >> 2;
  const float4 *p4 = (const float4*)pred, *h4 = (const float4*)target, *l4 = (const float4*)cond;
  for (int64_t i = gid; i < nv; i += stride) {
    const float4 p = p4[i], h = h4[i];
    mon_add(m, p.x, h.x), mon_add(m, p.y, h.y), mon_add(m, p.z, h.z), mon_add(m, p.w, h.w);
    if (cond) {
      const float4 l = l4[i];
      mon_add_cond(m, l.x), mon_add_cond(m, l.y), mon_add_cond(m, l.z), mon_add_cond(m, l.w);
    }
  }
  if (gid < (n & 3)) {                       // the elements behind the last whole vector
    const int64_t i = nv * 4 + gid;
    mon_add(m, pred[i], target[i]);
    if (cond) mon_add_cond(m, cond[i]);
  }
  mon_block_reduce(m, sh);
  if (threadIdx.x == 0)
    for (int q = 0; q < MON_SUMS; ++q) partial[(size_t)blockIdx.x * MON_SUMS + q] = m.a[q];
}

__global__ __launch_bounds__(MON_THREADS) void train_monitor_final_kernel(const double* __restrict__ partial,
                                                                          double* __restrict__ out) {
  __shared__ double sh[MON_THREADS / 64][MON_SUMS];
  Mon m = {};
  for (int k = threadIdx.x; k < MON_BLOCKS; k += MON_THREADS)
    for (int q = 0; q < MON_SUMS; ++q) m.a[q] += partial[(size_t)k * MON_SUMS + q];
  mon_block_reduce(m, sh);
  if (threadIdx.x == 0)
    for (int q = 0; q < MON_SUMS; ++q) out[q] = m.a[q];
}

}  // namespace

hipError_t latent_gather_launch(const void* const* hr_src, const void* const* lr_src, const int64_t* len, const int64_t* start,
                                const float* hr_mean, const float* hr_std, const float* lr_mean, const float* lr_std,
                                float* hr_out, float* lr_out, int B, int C, int T, hipStream_t s) {
  const int64_t rows2 = 2 * (int64_t)B * C;
  if (rows2 <= 0 || T <= 0) return hipSuccess;
  const int row_halves = (T + 14 + 7) / 8 * 8;   // the crop, up to 7 halves ahead of it and up to 7 behind, in whole 16-byte chunks
  const size_t lds = (size_t)DT_ROWS * row_halves * sizeof(unsigned short);
  const dim3 grid((unsigned)((rows2 + DT_ROWS - 1) / DT_ROWS)), block(DT_THREADS);
  if (T % 4 == 0)
    hipLaunchKernelGGL(latent_gather_kernel<4>, grid, block, lds, s, hr_src, lr_src, len, start, hr_mean, hr_std, lr_mean,
                       lr_std, hr_out, lr_out, B, C, T, row_halves);
  else
    hipLaunchKernelGGL(latent_gather_kernel<2>, grid, block, lds, s, hr_src, lr_src, len, start, hr_mean, hr_std, lr_mean,
                       lr_std, hr_out, lr_out, B, C, T, row_halves);
  return hipGetLastError();
}

hipError_t train_monitor_launch(const float* pred, const float* target, const float* cond, int64_t n, double* partial,
                                double* out, hipStream_t s) {
  hipLaunchKernelGGL(train_monitor_partial_kernel, dim3(MON_BLOCKS), dim3(MON_THREADS), 0, s, pred, target, cond, n, partial);
  hipLaunchKernelGGL(train_monitor_final_kernel, dim3(1), dim3(MON_THREADS), 0, s, partial, out);
  return hipGetLastError();
}
