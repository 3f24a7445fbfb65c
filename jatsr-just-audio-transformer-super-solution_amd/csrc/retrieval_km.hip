// k-means compaction of a retrieval bank for gfx950: the assignment of pool rows to centroids, the centroid
// update and the inertia.  fp16 MFMA by intrinsic in both operand-dtype builds, like retrieval.hip.
//
// Assignment.  d(n, i) = (|q_n|^2 + |k_i|^2) - 2 q_n.k_i with the stored fp32 norms; both operands are fp16 rows, so the product
// is ONE v_mfma_f32_32x32x16_f16 pass per 16-channel step (the search's second pass carries the low half of an fp32 query; a
// pool row has none).  The roles are the search's: centroids are the A operand (rows), pool rows the B operand (columns), so a
// lane owns pool rows (lane & 31) and (lane & 31) + 32 and 16 centroid rows of the tile, and the running (d, idx) of each is a
// per-lane compare.  What changes is the shape: the pool is the large side, so a workgroup keeps KM_QTILE = 64 pool rows in LDS
// (one fp16 plane: the bytes the search spends on the hi and lo planes of 32 queries) and streams ALL K centroids past them in
// tiles of RT_KTILE rows, RT_KCHUNK channels at a time, every A fragment used for two MFMAs.  No split of K over workgroups,
// so no partials, no workspace and no second kernel; the centroid stream (K C 2 bytes, 20 MB at K = 10 000, C = 1024) is read
// once per 64 pool rows and stays in the L2 / MALL.  The pool is read once, row-major, 16 bytes per lane.
// Every d(n, i) is the same chain (channel steps ascending from zero) wherever it is computed, and the arg-min is taken by
// (d, index), so the result of a row does not depend on first / count, on the row's place in its tile or on the run.
// Edges: centroid rows >= K are neither read nor compared; pool rows >= count are zeros and are not written.
//
// Update.  Histogram of idx by integer atomics, exclusive scan (one workgroup), scatter of member indices by integer atomics
// (the order inside a cluster varies from run to run), then km_sum_kernel: one workgroup per (cluster, KM_CTILE channels,
// keys | values) whose four waves walk the member list, a wave reading 256 contiguous bytes of a member row, and keep exact
// int64 sums of the fp16 values in units of 2^-24 in registers.  Integer sums are exact, so the member order cannot reach the
// result.  mean = fp16(fp32(double(S) / double(n)) 2^-24): one rounding per conversion, the division correctly rounded.
#include "jat_retrieval_km_kernels.h"

typedef __attribute__((ext_vector_type(8))) _Float16 km_f16x8;
typedef __attribute__((ext_vector_type(16))) float km_f32x16;

namespace {

constexpr int KM_PREFETCH = 4;        // centroid chunks in flight per thread: 4 x 16 bytes each
constexpr int KROW = RT_KCHUNK + 8;   // halves per centroid row of the LDS tile: 144 bytes, 16-byte aligned, rows 4 banks apart

__device__ __forceinline__ bool better(float d, int i, float bd, int bi) { return d < bd || (d == bd && i < bi); }

__global__ __launch_bounds__(RT_THREADS) void km_assign_kernel(const uint16_t* __restrict__ pool,
                                                               const float* __restrict__ pnorms, int64_t first, int count,
                                                               const uint16_t* __restrict__ keys,
                                                               const float* __restrict__ norms, int K, int C, int32_t* idx,
                                                               float* __restrict__ dist2, int32_t* __restrict__ changed) {
  extern __shared__ uint4 km_lds[];
  const int Cp = (C + RT_KCHUNK - 1) / RT_KCHUNK * RT_KCHUNK;   // whole chunks: channels [C, Cp) are zeros on both sides
  const int QS = Cp + 8;                                  // halves per pool row: 16-byte aligned, rows 4 banks apart
  uint16_t* sQ = (uint16_t*)km_lds;                       // [KM_QTILE][QS]
  uint16_t* sK = sQ + KM_QTILE * QS;                      // [RT_KTILE][KROW]; the candidates of the final compare afterwards
  float* qn = (float*)(sK + RT_KTILE * KROW);             // [KM_QTILE]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q0 = blockIdx.x * KM_QTILE;

  // the pool rows of this tile, as they are stored: 16 bytes per lane along the row; rows behind the range are zeros
  {
    const int per = C / 8, perp = Cp / 8;
    for (int e = tid; e < KM_QTILE * perp; e += RT_THREADS) {
      const int r = e / perp, c8 = e - r * perp;
      uint4 v = uint4{0u, 0u, 0u, 0u};
      if (q0 + r < count && c8 < per) v = *(const uint4*)(pool + (first + q0 + r) * (int64_t)C + c8 * 8);
      *(uint4*)(sQ + r * QS + c8 * 8) = v;
    }
    if (tid < KM_QTILE) qn[tid] = q0 + tid < count ? pnorms[first + q0 + tid] : 0.f;
  }
  // (the loop's first barrier orders qn and the plane before their first read)

  const int ntiles = (K + RT_KTILE - 1) / RT_KTILE, nch = Cp / RT_KCHUNK;
  const int total = ntiles * nch;
  const int col = lane & 31, half = lane >> 5;

  uint4 pre[KM_PREFETCH][4];
  const int frow = tid >> 3, fcol = (tid & 7) * 8;         // this thread's 16 bytes of centroid rows frow + 32 i of every chunk
  int f_tile = 0, f_ch = 0;                                // the next chunk to request
  auto fetch = [&](uint4 (&dst)[4]) {
    const int key = f_tile * RT_KTILE + frow, c = f_ch * RT_KCHUNK + fcol;
    const uint16_t* p = keys + (int64_t)key * C + c;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      dst[i] = (key + 32 * i < K && c < C) ? *(const uint4*)(p + (int64_t)(32 * i) * C) : uint4{0u, 0u, 0u, 0u};
    if (++f_ch == nch) f_ch = 0, ++f_tile;
  };

  float best_d[2] = {__builtin_inff(), __builtin_inff()};
  int best_i[2] = {0, 0};
  int tile = 0, ch = 0;                                    // the chunk in LDS
  km_f32x16 acc0, acc1;
#pragma unroll
  for (int j = 0; j < KM_PREFETCH; ++j)
    if (j < total) fetch(pre[j]);
  for (int it0 = 0; it0 < total; it0 += KM_PREFETCH) {
#pragma unroll
    for (int j = 0; j < KM_PREFETCH; ++j) {
      const int it = it0 + j;
      if (it >= total) break;                              // uniform over the workgroup
      __syncthreads();
#pragma unroll
      for (int i = 0; i < 4; ++i) *(uint4*)(sK + (frow + 32 * i) * KROW + fcol) = pre[j][i];
      __syncthreads();
      if (it + KM_PREFETCH < total) fetch(pre[j]);
      if (ch == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc0[r] = 0.f, acc1[r] = 0.f;
      }
      km_f16x8 a[RT_KCHUNK / 16], b0[RT_KCHUNK / 16], b1[RT_KCHUNK / 16];
#pragma unroll
      for (int ks = 0; ks < RT_KCHUNK / 16; ++ks) {
        const int kk = ks * 16 + 8 * half;
        a[ks] = *(const km_f16x8*)(sK + (wave * 32 + col) * KROW + kk);
        b0[ks] = *(const km_f16x8*)(sQ + col * QS + ch * RT_KCHUNK + kk);
        b1[ks] = *(const km_f16x8*)(sQ + (col + 32) * QS + ch * RT_KCHUNK + kk);
      }
#pragma unroll
      for (int ks = 0; ks < RT_KCHUNK / 16; ++ks) {          // ascending 16-channel steps
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[ks], b0[ks], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[ks], b1[ks], acc1, 0, 0, 0);
      }
      if (ch == nch - 1) {
        // acc[4 g + r] = q(col) . k(row 8 g + 4 half + r): rows ascend with the register, tiles with the loop, so a strict <
        // keeps the lowest index of a lane's rows on equal d
        const float qv0 = qn[col], qv1 = qn[col + 32];
        const int kbase = tile * RT_KTILE + wave * 32 + 4 * half;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int k0 = kbase + 8 * g;
          const float4 kn = *(const float4*)(norms + k0);    // norms has whole RT_KTILE groups allocated
          const float kv[4] = {kn.x, kn.y, kn.z, kn.w};
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float d0 = (qv0 + kv[r]) - 2.f * acc0[4 * g + r];
            const float d1 = (qv1 + kv[r]) - 2.f * acc1[4 * g + r];
            if (k0 + r < K && d0 < best_d[0]) best_d[0] = d0, best_i[0] = k0 + r;
            if (k0 + r < K && d1 < best_d[1]) best_d[1] = d1, best_i[1] = k0 + r;
          }
        }
        ch = 0, ++tile;
      } else {
        ++ch;
      }
    }
  }

  // the eight candidates of a pool row (4 waves x 2 halves own disjoint centroid rows): the least by (d, index)
  __syncthreads();
  RtPartial* cand = (RtPartial*)sK;                        // [8][KM_QTILE]
  cand[(wave * 2 + half) * KM_QTILE + col] = RtPartial{best_d[0], best_i[0]};
  cand[(wave * 2 + half) * KM_QTILE + col + 32] = RtPartial{best_d[1], best_i[1]};
  __syncthreads();
  if (tid < KM_QTILE) {                                    // wave 0, whole
    RtPartial b = cand[tid];
#pragma unroll
    for (int k = 1; k < 8; ++k) {
      const RtPartial c = cand[k * KM_QTILE + tid];
      if (better(c.d, c.idx, b.d, b.idx)) b = c;
    }
    const int g = q0 + tid;
    bool diff = false;
    if (g < count) {
      diff = idx[g] != b.idx;                              // what the buffer held on entry
      idx[g] = b.idx;
      if (dist2) dist2[g] = b.d > 0.f ? b.d : 0.f;
    }
    const unsigned long long moved = __ballot(diff);
    if (changed && tid == 0 && moved) atomicAdd(changed, (int)__popcll(moved));
  }
}

// ---- update ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RT_THREADS) void km_zero_kernel(int32_t* __restrict__ p, int n) {
  const int i = blockIdx.x * RT_THREADS + threadIdx.x;
  if (i < n) p[i] = 0;
}

__global__ __launch_bounds__(RT_THREADS) void km_hist_kernel(const int32_t* __restrict__ idx, int N, int K,
                                                             int32_t* __restrict__ counts) {
  const int n = blockIdx.x * RT_THREADS + threadIdx.x;
  if (n >= N) return;
  const int i = idx[n];
  if ((unsigned)i < (unsigned)K) atomicAdd(&counts[i], 1);   // an index outside [0, K) joins no cluster
}

// offsets[i] = cursor[i] = counts[0] + .. + counts[i - 1]: one workgroup, a contiguous run of clusters per thread
constexpr int KM_SCAN_THREADS = 1024;
__global__ __launch_bounds__(KM_SCAN_THREADS) void km_scan_kernel(const int32_t* __restrict__ counts, int K,
                                                                  int32_t* __restrict__ offsets, int32_t* __restrict__ cursor) {
  __shared__ int part[KM_SCAN_THREADS];
  const int tid = threadIdx.x;
  const int per = (K + KM_SCAN_THREADS - 1) / KM_SCAN_THREADS;
  const int lo = min(K, tid * per), hi = min(K, lo + per);
  int s = 0;
  for (int i = lo; i < hi; ++i) s += counts[i];
  part[tid] = s;
  __syncthreads();
  for (int off = 1; off < KM_SCAN_THREADS; off <<= 1) {
    const int v = tid >= off ? part[tid - off] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  int base = part[tid] - s;
  for (int i = lo; i < hi; ++i) {
    offsets[i] = base, cursor[i] = base;
    base += counts[i];
  }
}

__global__ __launch_bounds__(RT_THREADS) void km_scatter_kernel(const int32_t* __restrict__ idx, int N, int K,
                                                                int32_t* __restrict__ cursor, int32_t* __restrict__ members) {
  const int n = blockIdx.x * RT_THREADS + threadIdx.x;
  if (n >= N) return;
  const int i = idx[n];
  if ((unsigned)i < (unsigned)K) members[atomicAdd(&cursor[i], 1)] = n;   // a place below offsets[i] + counts[i] <= N
}

// a finite fp16 value in units of 2^-24: an integer of magnitude below 2^40
__device__ __forceinline__ long long h2units(uint32_t h) {
  const int e = (h >> 10) & 31, m = h & 1023;
  const long long v = e ? (long long)(1024 + m) << (e - 1) : (long long)m;
  return (h & 0x8000u) ? -v : v;
}

__global__ __launch_bounds__(RT_THREADS) void km_sum_kernel(const uint16_t* __restrict__ pkeys,
                                                            const uint16_t* __restrict__ pvals,
                                                            const int32_t* __restrict__ members,
                                                            const int32_t* __restrict__ offsets,
                                                            const int32_t* __restrict__ counts, uint16_t* __restrict__ ckeys,
                                                            uint16_t* __restrict__ cvals, int C) {
  __shared__ long long red[RT_THREADS / 64][KM_CTILE];
  const int i = blockIdx.x, c0 = blockIdx.y * KM_CTILE;
  const int n = counts[i];
  if (n == 0) return;                                      // an empty cluster keeps its row (uniform over the workgroup)
  const uint16_t* rows = blockIdx.z ? pvals : pkeys;
  uint16_t* out = blockIdx.z ? cvals : ckeys;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = c0 + 2 * lane;
  const int32_t* m = members + offsets[i];
  long long s0 = 0, s1 = 0;
  if (c < C) {                                             // C is even: both halves of the pair are inside
    const uint16_t* base = rows + c;
    int j = wave;
    for (; j + 12 < n; j += 16) {                          // four member rows in flight per wave
      uint32_t v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = *(const uint32_t*)(base + (int64_t)m[j + 4 * u] * C);
#pragma unroll
      for (int u = 0; u < 4; ++u) s0 += h2units(v[u] & 0xffffu), s1 += h2units(v[u] >> 16);
    }
    for (; j < n; j += 4) {
      const uint32_t v = *(const uint32_t*)(base + (int64_t)m[j] * C);
      s0 += h2units(v & 0xffffu), s1 += h2units(v >> 16);
    }
  }
  red[wave][2 * lane] = s0, red[wave][2 * lane + 1] = s1;
  __syncthreads();
  if (tid < KM_CTILE && c0 + tid < C) {
    const long long S = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);   // exact in any order
    const double q = (double)S / (double)n;                // int64 -> double to nearest even, the division correctly rounded
    const float f = (float)q * 0x1p-24f;                   // to nearest even; the scaling is exact
    out[(int64_t)i * C + c0 + tid] = __builtin_bit_cast(uint16_t, (_Float16)f);
  }
}

// ---- inertia: strided fp64 partial sums in ascending order, then a fixed tree ---------------------------------------------------
__global__ __launch_bounds__(KM_SCAN_THREADS) void km_sum_dist2_kernel(const float* __restrict__ d, int64_t n,
                                                                       double* __restrict__ out) {
  __shared__ double part[KM_SCAN_THREADS];
  const int tid = threadIdx.x;
  double s = 0.0;
#pragma unroll 8
  for (int64_t i = tid; i < n; i += KM_SCAN_THREADS) s += (double)d[i];
  part[tid] = s;
  __syncthreads();
  for (int off = KM_SCAN_THREADS / 2; off > 0; off >>= 1) {
    if (tid < off) part[tid] += part[tid + off];
    __syncthreads();
  }
  if (tid == 0) out[0] = part[0];
}

size_t assign_lds_bytes(int C) {
  const int Cp = (C + RT_KCHUNK - 1) / RT_KCHUNK * RT_KCHUNK;
  return (size_t)(KM_QTILE * (Cp + 8) + RT_KTILE * KROW) * sizeof(uint16_t) + (size_t)KM_QTILE * sizeof(float);
}

}  // namespace

hipError_t km_assign_launch(const uint16_t* pool, const float* pnorms, int64_t first, int count, const uint16_t* cent,
                            const float* cnorms, int K, int C, int32_t* idx, float* dist2, int32_t* changed, hipStream_t s) {
  static_assert(KROW % 8 == 0 && sizeof(RtPartial) == 8 && 8 * KM_QTILE * sizeof(RtPartial) <= RT_KTILE * KROW * 2,
                "LDS layout of km_assign_kernel: the eight candidates of every pool row fit the centroid tile");
  static_assert(RT_KTILE * (RT_KCHUNK / 8) == 4 * RT_THREADS && RT_KTILE == 32 * (RT_THREADS / 64) && KM_QTILE == 64,
                "tile loader and fragment owners of km_assign_kernel");
  if (count <= 0) return hipSuccess;
  static const hipError_t attr = hipFuncSetAttribute((const void*)km_assign_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     (int)assign_lds_bytes(RT_MAX_C));
  if (attr != hipSuccess) return attr;
  hipLaunchKernelGGL(km_assign_kernel, dim3((unsigned)((count + KM_QTILE - 1) / KM_QTILE)), dim3(RT_THREADS), assign_lds_bytes(C),
                     s, pool, pnorms, first, count, cent, cnorms, K, C, idx, dist2, changed);
  return hipGetLastError();
}

hipError_t km_update_launch(const uint16_t* pkeys, const uint16_t* pvals, const int32_t* idx, int N, uint16_t* ckeys,
                            uint16_t* cvals, int K, int C, int32_t* counts, int32_t* offsets, int32_t* cursor,
                            int32_t* members, hipStream_t s) {
  static_assert(KM_CTILE == 2 * 64, "km_sum_kernel: a wave covers the channel tile with two halves per lane");
  const dim3 block(RT_THREADS);
  const unsigned nb = (unsigned)((N + RT_THREADS - 1) / RT_THREADS);
  hipLaunchKernelGGL(km_zero_kernel, dim3((unsigned)((K + RT_THREADS - 1) / RT_THREADS)), block, 0, s, counts, K);
  hipLaunchKernelGGL(km_hist_kernel, dim3(nb), block, 0, s, idx, N, K, counts);
  hipLaunchKernelGGL(km_scan_kernel, dim3(1), dim3(KM_SCAN_THREADS), 0, s, counts, K, offsets, cursor);
  hipLaunchKernelGGL(km_scatter_kernel, dim3(nb), block, 0, s, idx, N, K, cursor, members);
  hipLaunchKernelGGL(km_sum_kernel, dim3((unsigned)K, (unsigned)((C + KM_CTILE - 1) / KM_CTILE), pvals ? 2u : 1u), block, 0, s,
                     pkeys, pvals, members, offsets, counts, ckeys, cvals, C);
  return hipGetLastError();
}

hipError_t km_sum_dist2_launch(const float* d, int64_t n, double* out, hipStream_t s) {
  hipLaunchKernelGGL(km_sum_dist2_kernel, dim3(1), dim3(KM_SCAN_THREADS), 0, s, d, n, out);
  return hipGetLastError();
}
