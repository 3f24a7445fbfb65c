// IVF index over a retrieval bank for gfx950: the grouping of a bank's rows by list and the scan of the probed
// lists.  fp16 MFMA by intrinsic in both operand-dtype builds, like retrieval.hip.
//
// Grouping.  Histogram of idx by integer atomics (rows whose idx is outside [0, nlist) count for a virtual list `nlist` behind
// all others), exclusive scan (one workgroup) -> offsets, scatter of member rows by integer atomics (the order inside a list
// varies from run to run), then ivf_rank_kernel: the place of a member inside its list is the number of smaller members, an
// integer count that no scheduling can change, so order is the stable sort of the rows by idx on every run.  ivf_gather_kernel
// copies keys, values and norms 16 bytes per lane.
//
// Search.  d(q, p) is the chain of bank_search_kernel (retrieval.hip), restated: the query normalised with the expression of
// channel_affine_kernel and split hi = fp16(q), lo = fp16(q - hi); |q|^2 as eight phase sums (fmaf chains over channels cg,
// cg + 8, ..) added in ascending phase order; the product as v_mfma_f32_32x32x16_f16 over ascending 16-channel steps of the
// channels padded with zeros to whole RT_KCHUNK groups, hi before lo, into one fp32 accumulator, keys the A operand and the
// query the B operand; d = (|q|^2 + |k_p|^2) - 2 q.k_p.
// ivf_prepare_kernel does the query side once per call into row-major planes [nq, Cp] x 2 and qn [nq] (lanes along t on the
// read, 16 bytes per lane along the channels on the write).  ivf_scan_kernel is one workgroup per query: its four waves take
// the 32-row tiles of the probed lists in turn (a tile never crosses a list), each lane reading 16 bytes of ITS key row per
// 16-channel step straight from memory, one RT_KCHUNK group of loads in flight under the MFMAs of the one before; the query
// is broadcast to all 32 B columns from LDS, so every column holds the same products and the lanes of column 0 keep the KP
// best (d, position) pairs in registers.  The scan is bound by reading the lists, not by the MFMAs: the 31 idle columns cost
// nothing that matters.  The eight lists of the query are merged by (d, position) by one thread.
// Edges: a list boundary falls anywhere, so the norm of a row is read on its own (no float4 from a tile's first row); rows
// at or behind a list's end are neither read nor compared; a probe entry outside [0, nlist) probes nothing; offsets are
// clipped to [0, size] before they are used as addresses.
#include "jat_retrieval_ivf_kernels.h"

typedef __attribute__((ext_vector_type(8))) _Float16 ivf_f16x8;
typedef __attribute__((ext_vector_type(16))) float ivf_f32x16;

namespace {

constexpr int IVF_STEPS = RT_KCHUNK / 16;   // MFMA steps per group of key loads
constexpr int IVF_PROW = RT_KCHUNK + 8;     // halves per query row of the preparation's LDS tile: 144 bytes

__device__ __forceinline__ bool better(float d, int i, float bd, int bi) { return d < bd || (d == bd && i < bi); }

// The sorted list of one lane or of one query: KP (d, position) pairs ascending, unused places (+inf, -1).  The candidate
// lands in front of every entry it is `better` than.  Every index is a compile-time constant: the list stays in registers.
template <int KP>
__device__ __forceinline__ void list_insert(float (&ld)[KP], int (&li)[KP], float d, int i) {
#pragma unroll
  for (int j = KP - 1; j >= 1; --j) {
    const bool here = better(d, i, ld[j], li[j]), above = better(d, i, ld[j - 1], li[j - 1]);
    ld[j] = here ? (above ? ld[j - 1] : d) : ld[j];
    li[j] = here ? (above ? li[j - 1] : i) : li[j];
  }
  if (better(d, i, ld[0], li[0])) ld[0] = d, li[0] = i;
}

// ---- grouping ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RT_THREADS) void ivf_zero_kernel(int32_t* __restrict__ p, int n) {
  const int i = blockIdx.x * RT_THREADS + threadIdx.x;
  if (i < n) p[i] = 0;
}

// the list of a row: an index outside [0, nlist) is the virtual list nlist and is never used as an address
__device__ __forceinline__ int list_of(int i, int nlist) { return (unsigned)i < (unsigned)nlist ? i : nlist; }

__global__ __launch_bounds__(RT_THREADS) void ivf_hist_kernel(const int32_t* __restrict__ idx, int N, int nlist,
                                                              int32_t* __restrict__ counts) {
  const int n = blockIdx.x * RT_THREADS + threadIdx.x;
  if (n < N) atomicAdd(&counts[list_of(idx[n], nlist)], 1);
}

// offsets[i] = cursor[i] = counts[0] + .. + counts[i - 1] for i <= nlist (n = nlist + 1 entries; the counts arrive in cursor):
// one workgroup, a contiguous run of lists per thread
constexpr int IVF_SCAN_THREADS = 1024;
__global__ __launch_bounds__(IVF_SCAN_THREADS) void ivf_scan_offsets_kernel(int32_t* __restrict__ cursor, int n,
                                                                            int32_t* __restrict__ offsets) {
  __shared__ int part[IVF_SCAN_THREADS];
  const int tid = threadIdx.x;
  const int per = (n + IVF_SCAN_THREADS - 1) / IVF_SCAN_THREADS;
  const int lo = min(n, tid * per), hi = min(n, lo + per);
  int s = 0;
  for (int i = lo; i < hi; ++i) s += cursor[i];
  part[tid] = s;
  __syncthreads();
  for (int off = 1; off < IVF_SCAN_THREADS; off <<= 1) {
    const int v = tid >= off ? part[tid - off] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  int base = part[tid] - s;
  for (int i = lo; i < hi; ++i) {
    const int c = cursor[i];
    offsets[i] = base, cursor[i] = base;
    base += c;
  }
}

__global__ __launch_bounds__(RT_THREADS) void ivf_scatter_kernel(const int32_t* __restrict__ idx, int N, int nlist,
                                                                 int32_t* __restrict__ cursor, int32_t* __restrict__ members) {
  const int n = blockIdx.x * RT_THREADS + threadIdx.x;
  if (n < N) members[atomicAdd(&cursor[list_of(idx[n], nlist)], 1)] = n;   // a place below offsets[l] + counts[l] <= N
}

// order[offsets[l] + (members of l below n)] = n: an integer count, the same whatever order the scatter left
__global__ __launch_bounds__(RT_THREADS) void ivf_rank_kernel(const int32_t* __restrict__ idx, int N, int nlist,
                                                              const int32_t* __restrict__ offsets,
                                                              const int32_t* __restrict__ members, int32_t* __restrict__ order) {
  const int n = blockIdx.x * RT_THREADS + threadIdx.x;
  if (n >= N) return;
  const int l = list_of(idx[n], nlist);
  const int b = offsets[l], e = l == nlist ? N : offsets[l + 1];
  int r = 0;
  for (int j = b; j < e; ++j) r += members[j] < n ? 1 : 0;
  order[b + r] = n;
}

// dst row p = src row order[p]: 16 bytes per thread, keys (blockIdx.y = 0, with the norm) and values (1)
__global__ __launch_bounds__(RT_THREADS) void ivf_gather_kernel(const uint16_t* __restrict__ skeys,
                                                                const uint16_t* __restrict__ svals,
                                                                const float* __restrict__ snorms,
                                                                const int32_t* __restrict__ order, int N, int C,
                                                                uint16_t* __restrict__ dkeys, uint16_t* __restrict__ dvals,
                                                                float* __restrict__ dnorms) {
  const int per = C / 8;
  const int64_t e = (int64_t)blockIdx.x * RT_THREADS + threadIdx.x;
  const int64_t p = e / per;
  if (p >= N) return;
  const int c8 = (int)(e - p * per);
  const int src = order[p];
  if ((unsigned)src >= (unsigned)N) return;                  // order is this call's own output: a guard, not a case
  const uint16_t* in = blockIdx.y ? svals : skeys;
  uint16_t* out = blockIdx.y ? dvals : dkeys;
  *(uint4*)(out + p * C + c8 * 8) = *(const uint4*)(in + (int64_t)src * C + c8 * 8);
  if (blockIdx.y == 0 && c8 == 0) dnorms[p] = snorms[src];
}

// ---- search: the query side ----------------------------------------------------------------------------------------------------
// 32 queries per workgroup, lanes along t, eight channel phases: the loop of bank_search_kernel, one RT_KCHUNK group of channels
// at a time through LDS so that the planes are written 16 bytes per lane
template <bool NORM>
__global__ __launch_bounds__(RT_THREADS) void ivf_prepare_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                                 const float* __restrict__ sd, int C, int T, int64_t nq,
                                                                 uint16_t* __restrict__ qhi, uint16_t* __restrict__ qlo,
                                                                 float* __restrict__ qn) {
  __shared__ uint4 tile4[2 * RT_QTILE * IVF_PROW / 8];
  __shared__ float qpart[8][RT_QTILE];
  uint16_t* thi = (uint16_t*)tile4;                          // [RT_QTILE][IVF_PROW]
  uint16_t* tlo = thi + RT_QTILE * IVF_PROW;                 // [RT_QTILE][IVF_PROW]
  const int Cp = (C + RT_KCHUNK - 1) / RT_KCHUNK * RT_KCHUNK;
  const int tid = threadIdx.x, qi = tid & 31, cg = tid >> 5;
  const int64_t g = (int64_t)blockIdx.x * RT_QTILE + qi;
  const bool live = g < nq;
  const int64_t gc = live ? g : nq - 1, b = gc / T, t = gc - b * T;
  const float* xp = x + b * C * T + t;
  const int orow = tid >> 3, ocol = (tid & 7) * 8;           // this thread's 16 bytes of the tile on the way out
  const int64_t og = (int64_t)blockIdx.x * RT_QTILE + orow;
  float s = 0.f;
  for (int c0 = 0; c0 < Cp; c0 += RT_KCHUNK) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int c = c0 + cg + 8 * u;
      v[u] = c < C ? xp[(int64_t)c * T] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int c = c0 + cg + 8 * u;
      uint16_t h16 = 0, l16 = 0;
      if (c < C) {
        const float q = NORM ? (v[u] - mean[c]) / sd[c] : v[u];   // the expression of channel_affine_kernel
        const _Float16 h = (_Float16)q;
        const _Float16 l = (_Float16)(q - (float)h);
        h16 = __builtin_bit_cast(uint16_t, h), l16 = __builtin_bit_cast(uint16_t, l);
        s = fmaf(q, q, s);                                   // channels cg, cg + 8, ... in ascending order
      }
      thi[qi * IVF_PROW + cg + 8 * u] = h16;
      tlo[qi * IVF_PROW + cg + 8 * u] = l16;
    }
    __syncthreads();
    if (og < nq) {
      *(uint4*)(qhi + og * Cp + c0 + ocol) = *(const uint4*)(thi + orow * IVF_PROW + ocol);
      *(uint4*)(qlo + og * Cp + c0 + ocol) = *(const uint4*)(tlo + orow * IVF_PROW + ocol);
    }
    __syncthreads();
  }
  qpart[cg][qi] = s;
  __syncthreads();
  if (tid < RT_QTILE) {
    float a = qpart[0][tid];
#pragma unroll
    for (int k = 1; k < 8; ++k) a += qpart[k][tid];
    const int64_t gq = (int64_t)blockIdx.x * RT_QTILE + tid;
    if (gq < nq) qn[gq] = a;
  }
}

// ---- search: the scan of the probed lists --------------------------------------------------------------------------------------
template <int KP>
__global__ __launch_bounds__(RT_THREADS) void ivf_scan_kernel(const uint16_t* __restrict__ keys, const float* __restrict__ norms,
                                                              int size, int C, const int32_t* __restrict__ offsets, int nlist,
                                                              const int32_t* __restrict__ probes, int nprobe,
                                                              const uint16_t* __restrict__ qhi, const uint16_t* __restrict__ qlo,
                                                              const float* __restrict__ qn, int k, int32_t* __restrict__ idx,
                                                              float* __restrict__ dist2) {
  __shared__ uint4 plane4[2 * RT_MAX_C / 8];
  __shared__ RtPartial cand[8][KP];
  const int Cp = (C + RT_KCHUNK - 1) / RT_KCHUNK * RT_KCHUNK, nch = Cp / RT_KCHUNK;
  uint16_t* sh = (uint16_t*)plane4;                          // [Cp]
  uint16_t* sl = sh + RT_MAX_C;                              // [Cp]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 31, half = lane >> 5;
  const int64_t g = blockIdx.x;
  {
    const int piece = tid & 127;
    if (piece < Cp / 8) {
      const uint16_t* src = (tid < 128 ? qhi : qlo) + g * Cp + piece * 8;
      *(uint4*)((tid < 128 ? sh : sl) + piece * 8) = *(const uint4*)src;
    }
  }
  __syncthreads();
  const float qv = qn[g];

  float ld[KP];
  int li[KP];
#pragma unroll
  for (int j = 0; j < KP; ++j) ld[j] = __builtin_inff(), li[j] = -1;

  // the tiles of the probed lists, numbered through the lists in probe order: wave w takes tiles w, w + 4, ...
  int item = wave;
  for (int j = 0; j < nprobe; ++j) {
    const int l = probes[g * nprobe + j];
    if ((unsigned)l >= (unsigned)nlist) continue;            // -1: fewer lists than probes
    const int b = min(max(offsets[l], 0), size), e = min(max(offsets[l + 1], b), size);
    const int nt = (e - b + IVF_TILE - 1) / IVF_TILE;
    for (; item < nt; item += RT_THREADS / 64) {
      const int row0 = b + item * IVF_TILE;                  // < e
      const bool mine = row0 + col < e;                      // this lane's key row exists
      const uint16_t* kp = keys + (int64_t)(mine ? row0 + col : row0) * C + 8 * half;
      auto fetch = [&](ivf_f16x8 (&dst)[IVF_STEPS], int ch) {
#pragma unroll
        for (int ks = 0; ks < IVF_STEPS; ++ks) {
          const int c = ch * RT_KCHUNK + ks * 16;            // C is a multiple of 32: a step is inside or outside as a whole
          ivf_f16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
          dst[ks] = (mine && c < C) ? *(const ivf_f16x8*)(kp + c) : z;
        }
      };
      ivf_f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      ivf_f16x8 cur[IVF_STEPS], nxt[IVF_STEPS];
      fetch(cur, 0);
      for (int ch = 0; ch < nch; ++ch) {
        if (ch + 1 < nch) fetch(nxt, ch + 1);
        ivf_f16x8 bh[IVF_STEPS], bl[IVF_STEPS];
#pragma unroll
        for (int ks = 0; ks < IVF_STEPS; ++ks) {
          const int kk = ch * RT_KCHUNK + ks * 16 + 8 * half;
          bh[ks] = *(const ivf_f16x8*)(sh + kk);
          bl[ks] = *(const ivf_f16x8*)(sl + kk);
        }
#pragma unroll
        for (int ks = 0; ks < IVF_STEPS; ++ks) {             // ascending 16-channel steps, hi before lo
          acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur[ks], bh[ks], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur[ks], bl[ks], acc, 0, 0, 0);
        }
#pragma unroll
        for (int ks = 0; ks < IVF_STEPS; ++ks) cur[ks] = nxt[ks];
      }
      // acc[4 gq + r] = q . k(row0 + 8 gq + 4 half + r) in every column: column 0 keeps the lists
      if (col == 0) {
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int p = row0 + 8 * gq + 4 * half + r;
            if (p < e) {
              const float d = (qv + norms[p]) - 2.f * acc[4 * gq + r];
              if (better(d, p, ld[KP - 1], li[KP - 1])) list_insert<KP>(ld, li, d, p);
            }
          }
        }
      }
    }
    item -= nt;
  }

  // the eight lists of the query (4 waves x 2 halves), each ascending in (d, position), merged by (d, position)
  if (col == 0) {
#pragma unroll
    for (int j = 0; j < KP; ++j) cand[wave * 2 + half][j] = RtPartial{ld[j], li[j]};
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 8; ++w) {
#pragma unroll
      for (int j = 0; j < KP; ++j) {
        const RtPartial c = cand[w][j];
        if (!better(c.d, c.idx, ld[KP - 1], li[KP - 1])) break;   // the list ascends: nothing behind c enters either
        list_insert<KP>(ld, li, c.d, c.idx);
      }
    }
#pragma unroll
    for (int j = 0; j < KP; ++j) {
      if (j < k) {
        idx[g * k + j] = ld[j] == __builtin_inff() ? -1 : li[j];
        if (dist2) dist2[g * k + j] = ld[j] > 0.f ? ld[j] : 0.f;
      }
    }
  }
}

template <int KP>
void scan_launch(const uint16_t* keys, const float* norms, int size, int C, const int32_t* offsets, int nlist,
                 const int32_t* probes, int nprobe, const uint16_t* qhi, const uint16_t* qlo, const float* qn, int64_t nq, int k,
                 int32_t* idx, float* dist2, hipStream_t s) {
  hipLaunchKernelGGL(ivf_scan_kernel<KP>, dim3((unsigned)nq), dim3(RT_THREADS), 0, s, keys, norms, size, C, offsets, nlist,
                     probes, nprobe, qhi, qlo, qn, k, idx, dist2);
}

}  // namespace

hipError_t ivf_group_launch(const uint16_t* skeys, const uint16_t* svals, const float* snorms, const int32_t* idx, int N,
                            int nlist, int C, uint16_t* dkeys, uint16_t* dvals, float* dnorms, int32_t* offsets,
                            int32_t* order, int32_t* cursor, int32_t* members, hipStream_t s) {
  const dim3 block(RT_THREADS);
  const unsigned nb = (unsigned)((N + RT_THREADS - 1) / RT_THREADS);
  hipLaunchKernelGGL(ivf_zero_kernel, dim3((unsigned)((nlist + 1 + RT_THREADS - 1) / RT_THREADS)), block, 0, s, cursor,
                     nlist + 1);
  hipLaunchKernelGGL(ivf_hist_kernel, dim3(nb), block, 0, s, idx, N, nlist, cursor);
  hipLaunchKernelGGL(ivf_scan_offsets_kernel, dim3(1), dim3(IVF_SCAN_THREADS), 0, s, cursor, nlist + 1, offsets);
  hipLaunchKernelGGL(ivf_scatter_kernel, dim3(nb), block, 0, s, idx, N, nlist, cursor, members);
  hipLaunchKernelGGL(ivf_rank_kernel, dim3(nb), block, 0, s, idx, N, nlist, offsets, members, order);
  const int64_t pieces = (int64_t)N * (C / 8);
  hipLaunchKernelGGL(ivf_gather_kernel, dim3((unsigned)((pieces + RT_THREADS - 1) / RT_THREADS), svals ? 2u : 1u), block, 0, s,
                     skeys, svals, snorms, order, N, C, dkeys, dvals, dnorms);
  return hipGetLastError();
}

hipError_t ivf_prepare_launch(const float* x, const float* mean, const float* std, int B, int T, int C, uint16_t* qhi,
                              uint16_t* qlo, float* qn, hipStream_t s) {
  static_assert(RT_QTILE * (RT_KCHUNK / 8) == RT_THREADS && RT_KCHUNK == 8 * 8 && IVF_PROW % 8 == 0,
                "tile of ivf_prepare_kernel: eight phases of eight channels in, 16 bytes per thread out");
  const int64_t nq = (int64_t)B * T;
  const dim3 grid((unsigned)((nq + RT_QTILE - 1) / RT_QTILE)), block(RT_THREADS);
  if (mean)
    hipLaunchKernelGGL(ivf_prepare_kernel<true>, grid, block, 0, s, x, mean, std, C, T, nq, qhi, qlo, qn);
  else
    hipLaunchKernelGGL(ivf_prepare_kernel<false>, grid, block, 0, s, x, mean, std, C, T, nq, qhi, qlo, qn);
  return hipGetLastError();
}

hipError_t ivf_scan_launch(const uint16_t* keys, const float* norms, int size, int C, const int32_t* offsets, int nlist,
                           const int32_t* probes, int nprobe, const uint16_t* qhi, const uint16_t* qlo, const float* qn,
                           int64_t nq, int k, int32_t* idx, float* dist2, hipStream_t s) {
  static_assert(RT_MAX_C % RT_KCHUNK == 0 && RT_MAX_C / 8 <= 128 && IVF_TILE == 32,
                "plane loader and tile of ivf_scan_kernel");
  switch (rt_list_length(k)) {
    case 1: scan_launch<1>(keys, norms, size, C, offsets, nlist, probes, nprobe, qhi, qlo, qn, nq, k, idx, dist2, s); break;
    case 2: scan_launch<2>(keys, norms, size, C, offsets, nlist, probes, nprobe, qhi, qlo, qn, nq, k, idx, dist2, s); break;
    case 4: scan_launch<4>(keys, norms, size, C, offsets, nlist, probes, nprobe, qhi, qlo, qn, nq, k, idx, dist2, s); break;
    default: scan_launch<8>(keys, norms, size, C, offsets, nlist, probes, nprobe, qhi, qlo, qn, nq, k, idx, dist2, s); break;
  }
  return hipGetLastError();
}
