// Latent retrieval kernels for gfx950: the fp16 bank (pack, norms), the exact nearest-neighbour search and the index-rate
// blend.  fp16 MFMA by intrinsic in both operand-dtype builds (the bank's rows are fp16 whatever the model's operands are).
//
// Search.  d(q, i) = |q|^2 + |k_i|^2 - 2 q.k_i over key rows [0, size), arg-min with the lowest index on equal d.  The key
// rows are exact fp16; the fp32 query is split q = hi + lo, hi = fp16(q), lo = fp16(q - hi), and the product runs as two
// v_mfma_f32_32x32x16_f16 passes (hi, then lo) per 16-channel step into one fp32 accumulator: the operand error is
// 2^-22 |q| instead of the 2^-11 |q| of one fp16 pass.  Keys are the A operand (rows), queries the B operand (columns), so
// a lane owns ONE query (lane & 31) and 16 key rows of the tile: the running (d, idx) is a per-lane compare with no cross-lane
// traffic until the end of the slab.
// A workgroup owns (RT_QTILE queries, one slab of RT_SLAB key rows).  It loads its queries once from x [B, C, T] (lanes
// along t: 128-byte lines), normalises and splits them, and keeps both planes in LDS for the whole slab; key tiles of
// RT_KTILE rows stream through LDS RT_KCHUNK channels at a time, the loads of the next four chunks in flight in registers
// under the MFMAs.
// Every d(q, i) is the same chain (channel steps ascending, hi before lo) wherever it is computed, so the result does not
// depend on the slab split, on B or on the query's place in its tile.  One partial per (slab, query); bank_reduce_kernel
// takes them in slab order.  No atomics.
// Edges: key rows >= size are neither read nor compared; queries >= B * T are zeros and are not written.
//
// Top-k.  The same scan with a list length KP of 2, 4 or 8 in place of the single (d, idx): a lane keeps its KP best pairs
// sorted in registers, the eight lists of a query are merged by (d, idx) in LDS at the end of the slab (KP partials per
// (slab, query)), and bank_reduce_topk_kernel merges the slabs' lists in slab order.  A request for k runs the next KP >= k
// and writes the first k entries.  bank_blend_topk_kernel mixes the k value rows with inverse-square-distance weights.
#include "jat_retrieval_kernels.h"

#include <type_traits>

typedef __attribute__((ext_vector_type(8))) _Float16 rt_f16x8;
typedef __attribute__((ext_vector_type(16))) float rt_f32x16;

namespace {

constexpr int RT_PREFETCH = 4;        // key chunks in flight per thread: 4 x 16 bytes each
constexpr int KROW = RT_KCHUNK + 8;   // halves per key row of the LDS tile: 144 bytes, 16-byte aligned, rows 4 banks apart

__device__ __forceinline__ uint16_t f2h(float f) { return __builtin_bit_cast(uint16_t, (_Float16)f); }
__device__ __forceinline__ float h2f(uint16_t h) { return (float)__builtin_bit_cast(_Float16, h); }

// ---- pack: [C, len] source frames -> fp16 rows --------------------------------------------------------------------------
// 32 frames x 32 channels per block through LDS: lanes along the frames on the read, along the channels on the write.
template <typename S>
__global__ __launch_bounds__(RT_THREADS) void bank_pack_kernel(const S* __restrict__ src, const S* __restrict__ src2,
                                                               int64_t len, int64_t first, int64_t stride, int count,
                                                               const float* __restrict__ mean, const float* __restrict__ sd,
                                                               const float* __restrict__ mean2, const float* __restrict__ sd2,
                                                               uint16_t* __restrict__ rows, uint16_t* __restrict__ rows2,
                                                               int64_t row0, int C) {
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
    const int64_t frame = first + (int64_t)i * stride;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = c0 + hi + 8 * k;
      tile[hi + 8 * k][lo] = ((float)in[(int64_t)c * len + frame] - mu[c]) / sg[c];   // the expression of channel_affine_kernel
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int j = f0 + hi + 8 * k;
    if (j < count) out[(row0 + j) * C + c0 + lo] = f2h(tile[lo][hi + 8 * k]);
  }
}

// ---- norms: one wave per row, lanes stride the channels, then a fixed shuffle tree ----------------------------------------
__global__ __launch_bounds__(RT_THREADS) void bank_norms_kernel(const uint16_t* __restrict__ rows, float* __restrict__ norms,
                                                                int64_t row0, int count, int C) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i = blockIdx.x * (RT_THREADS / 64) + wave;
  if (i >= count) return;
  const uint16_t* r = rows + (row0 + i) * C;
  float s = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float v = h2f(r[c]);
    s = fmaf(v, v, s);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if (lane == 0) norms[row0 + i] = s;
}

// ---- search ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool better(float d, int i, float bd, int bi) { return d < bd || (d == bd && i < bi); }

// The sorted list of one lane, of one query of a slab, of one query: KP (d, idx) pairs ascending, unused places (+inf, -1).
// `before(d, i, entry)` says whether the candidate goes in front of an entry; the candidate lands behind every entry it is
// not in front of.  Every index is a compile-time constant, so the list stays in registers.
template <int KP, typename Before>
__device__ __forceinline__ void list_insert(float (&ld)[KP], int (&li)[KP], float d, int i, Before before) {
#pragma unroll
  for (int j = KP - 1; j >= 1; --j) {
    const bool here = before(d, i, ld[j], li[j]), above = before(d, i, ld[j - 1], li[j - 1]);
    ld[j] = here ? (above ? ld[j - 1] : d) : ld[j];
    li[j] = here ? (above ? li[j - 1] : i) : li[j];
  }
  if (before(d, i, ld[0], li[0])) ld[0] = d, li[0] = i;
}

// KP = 1 is the arg-min search (one RtPartial per (slab, query), bank_reduce_kernel); KP = 2, 4, 8 keep the KP best per lane
// and write KP partials per (slab, query) for bank_reduce_topk_kernel.  The scan is the same text for all of them.
template <bool NORM, int KP>
__global__ __launch_bounds__(RT_THREADS) void bank_search_kernel(const uint16_t* __restrict__ keys,
                                                                 const float* __restrict__ norms, int size, int C,
                                                                 const float* __restrict__ x, const float* __restrict__ mean,
                                                                 const float* __restrict__ sd, int T, int64_t nq,
                                                                 RtPartial* __restrict__ part) {
  extern __shared__ uint4 rt_lds[];
  const int Cp = (C + RT_KCHUNK - 1) / RT_KCHUNK * RT_KCHUNK;   // whole chunks: channels [C, Cp) are zeros on both sides
  const int QS = Cp + 8;                                  // halves per query row: 16-byte aligned, rows 4 banks apart
  uint16_t* qhi = (uint16_t*)rt_lds;                      // [RT_QTILE][QS]
  uint16_t* qlo = qhi + RT_QTILE * QS;                    // [RT_QTILE][QS]
  uint16_t* sK = qlo + RT_QTILE * QS;                     // [RT_KTILE][KROW]; the candidates of the final compare afterwards
  float* qpart = (float*)(sK + RT_KTILE * KROW);          // [8][RT_QTILE]
  float* qn = qpart + 8 * RT_QTILE;                       // [RT_QTILE]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // the queries of this tile: lanes along t, eight channel phases; U loads in flight per lane (a lane behind the last
  // query reads the last query's address and keeps zeros)
  {
    const int qi = tid & 31, cg = tid >> 5;
    const int64_t g = (int64_t)blockIdx.x * RT_QTILE + qi;
    const bool live = g < nq;
    const int64_t gc = live ? g : nq - 1, b = gc / T, t = gc - b * T;
    const float* xp = x + b * C * T + t;
    float s = 0.f;
    for (int c = C + cg; c < Cp; c += 8) qhi[qi * QS + c] = qlo[qi * QS + c] = 0;
    auto batch = [&](int c0, auto u_tag) {
      constexpr int U = decltype(u_tag)::value;
      float v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) v[u] = xp[(int64_t)(c0 + 8 * u) * T];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int c = c0 + 8 * u;
        float q = NORM ? (v[u] - mean[c]) / sd[c] : v[u];    // the expression of channel_affine_kernel
        q = live ? q : 0.f;
        const _Float16 h = (_Float16)q;
        const _Float16 l = (_Float16)(q - (float)h);
        qhi[qi * QS + c] = __builtin_bit_cast(uint16_t, h);
        qlo[qi * QS + c] = __builtin_bit_cast(uint16_t, l);
        s = fmaf(q, q, s);                                   // channels cg, cg + 8, ... in ascending order
      }
    };
    int c = cg;
    for (; c + 8 * 16 <= C; c += 8 * 16) batch(c, std::integral_constant<int, 16>{});
    for (; c < C; c += 8 * 4) batch(c, std::integral_constant<int, 4>{});   // C / 8 is a multiple of four
    qpart[cg * RT_QTILE + qi] = s;
  }
  __syncthreads();
  if (tid < RT_QTILE) {
    float s = qpart[tid];
#pragma unroll
    for (int k = 1; k < 8; ++k) s += qpart[k * RT_QTILE + tid];
    qn[tid] = s;
  }
  // (the loop's first barrier orders qn and the planes before their first read)

  const int k_begin = blockIdx.y * RT_SLAB;
  const int k_end = min(size, k_begin + RT_SLAB);
  const int ntiles = (k_end - k_begin + RT_KTILE - 1) / RT_KTILE, nch = (C + RT_KCHUNK - 1) / RT_KCHUNK;
  const int total = ntiles * nch;
  const int col = lane & 31, half = lane >> 5;

  // RT_PREFETCH chunks of the key stream are in flight in registers: one chunk's MFMAs are far shorter than a trip to
  // memory, and a workgroup that fills the LDS has no neighbour on its CU to hide it
  uint4 pre[RT_PREFETCH][4];
  const int frow = tid >> 3, fcol = (tid & 7) * 8;         // this thread's 16 bytes of key rows frow + 32 i of every chunk
  int f_tile = 0, f_ch = 0;                                // the next chunk to request
  auto fetch = [&](uint4 (&dst)[4]) {
    const int key = k_begin + f_tile * RT_KTILE + frow, c = f_ch * RT_KCHUNK + fcol;
    const uint16_t* p = keys + (int64_t)key * C + c;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      dst[i] = (key + 32 * i < k_end && c < C) ? *(const uint4*)(p + (int64_t)(32 * i) * C) : uint4{0u, 0u, 0u, 0u};
    if (++f_ch == nch) f_ch = 0, ++f_tile;
  };

  float best_d = __builtin_inff();                         // KP == 1
  int best_i = k_begin;
  float ld[KP];                                            // KP > 1: rows ascend per lane, so a strict < keeps the lower
  int li[KP];                                              // index in front on equal d
#pragma unroll
  for (int j = 0; j < KP; ++j) ld[j] = __builtin_inff(), li[j] = -1;
  int tile = 0, ch = 0;                                    // the chunk in LDS
  rt_f32x16 acc;
#pragma unroll
  for (int j = 0; j < RT_PREFETCH; ++j)
    if (j < total) fetch(pre[j]);
  for (int it0 = 0; it0 < total; it0 += RT_PREFETCH) {
#pragma unroll
    for (int j = 0; j < RT_PREFETCH; ++j) {
      const int it = it0 + j;
      if (it >= total) break;                              // uniform over the workgroup
      __syncthreads();
#pragma unroll
      for (int i = 0; i < 4; ++i) *(uint4*)(sK + (frow + 32 * i) * KROW + fcol) = pre[j][i];
      __syncthreads();
      if (it + RT_PREFETCH < total) fetch(pre[j]);
      if (ch == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      }
      // every fragment of the chunk is requested before the first MFMA: one LDS round trip per chunk, not one per step
      rt_f16x8 a[RT_KCHUNK / 16], bh[RT_KCHUNK / 16], bl[RT_KCHUNK / 16];
#pragma unroll
      for (int ks = 0; ks < RT_KCHUNK / 16; ++ks) {
        const int kk = ks * 16 + 8 * half;
        a[ks] = *(const rt_f16x8*)(sK + (wave * 32 + col) * KROW + kk);
        bh[ks] = *(const rt_f16x8*)(qhi + col * QS + ch * RT_KCHUNK + kk);
        bl[ks] = *(const rt_f16x8*)(qlo + col * QS + ch * RT_KCHUNK + kk);
      }
#pragma unroll
      for (int ks = 0; ks < RT_KCHUNK / 16; ++ks) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[ks], bh[ks], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[ks], bl[ks], acc, 0, 0, 0);
      }
      if (ch == nch - 1) {
        // acc[4 g + r] = q(col) . k(row 8 g + 4 half + r): rows ascend with the register, tiles with the loop
        const float qv = qn[col];
        const int kbase = k_begin + tile * RT_KTILE + wave * 32 + 4 * half;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int k0 = kbase + 8 * g;
          const float4 kn = *(const float4*)(norms + k0);    // norms has whole RT_KTILE groups allocated
          const float kv[4] = {kn.x, kn.y, kn.z, kn.w};
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float d = (qv + kv[r]) - 2.f * acc[4 * g + r];
            if constexpr (KP == 1) {
              if (k0 + r < k_end && d < best_d) {
                best_d = d;
                best_i = k0 + r;
              }
            } else {
              if (k0 + r < k_end && d < ld[KP - 1])
                list_insert<KP>(ld, li, d, k0 + r, [](float d, int, float ed, int) { return d < ed; });
            }
          }
        }
        ch = 0, ++tile;
      } else {
        ++ch;
      }
    }
  }

  __syncthreads();
  RtPartial* cand = (RtPartial*)sK;                        // [8][KP][RT_QTILE]
  if constexpr (KP == 1) {
    cand[(wave * 2 + half) * RT_QTILE + col] = RtPartial{best_d, best_i};
    __syncthreads();
    if (tid < RT_QTILE) {
      RtPartial b = cand[tid];
#pragma unroll
      for (int k = 1; k < 8; ++k) {
        const RtPartial c = cand[k * RT_QTILE + tid];
        if (better(c.d, c.idx, b.d, b.idx)) b = c;
      }
      const int64_t g = (int64_t)blockIdx.x * RT_QTILE + tid;
      if (g < nq) part[(int64_t)blockIdx.y * nq + g] = b;
    }
  } else {
    // the eight lists of a query (4 waves x 2 halves), each ascending in (d, idx), merged by (d, idx) by one thread
#pragma unroll
    for (int j = 0; j < KP; ++j) cand[((wave * 2 + half) * KP + j) * RT_QTILE + col] = RtPartial{ld[j], li[j]};
    __syncthreads();
    if (tid < RT_QTILE) {
#pragma unroll
      for (int j = 0; j < KP; ++j) {
        const RtPartial c = cand[j * RT_QTILE + tid];
        ld[j] = c.d, li[j] = c.idx;
      }
      for (int l = 1; l < 8; ++l) {
#pragma unroll
        for (int j = 0; j < KP; ++j) {
          const RtPartial c = cand[(l * KP + j) * RT_QTILE + tid];
          if (!better(c.d, c.idx, ld[KP - 1], li[KP - 1])) break;   // the list ascends: nothing behind c enters either
          list_insert<KP>(ld, li, c.d, c.idx, [](float d, int i, float ed, int ei) { return better(d, i, ed, ei); });
        }
      }
      const int64_t g = (int64_t)blockIdx.x * RT_QTILE + tid;
      if (g < nq) {
#pragma unroll
        for (int j = 0; j < KP; ++j) part[((int64_t)blockIdx.y * nq + g) * KP + j] = RtPartial{ld[j], li[j]};
      }
    }
  }
}

__global__ __launch_bounds__(RT_THREADS) void bank_reduce_kernel(const RtPartial* __restrict__ part, int nslabs, int64_t nq,
                                                                 int32_t* __restrict__ idx, float* __restrict__ dist2) {
  const int64_t g = (int64_t)blockIdx.x * RT_THREADS + threadIdx.x;
  if (g >= nq) return;
  RtPartial b = part[g];
  for (int s = 1; s < nslabs; ++s) {
    const RtPartial c = part[(int64_t)s * nq + g];
    if (c.d < b.d) b = c;                                  // slabs ascend: an equal d keeps the lower index
  }
  idx[g] = b.idx;
  if (dist2) dist2[g] = b.d > 0.f ? b.d : 0.f;
}

// One thread per query: the slabs' lists in slab order.  Slabs ascend and a slab's list ascends in (d, idx), so a strict <
// keeps the lower index in front on equal d.  The first k of the KP entries are written; an unused place is (-1, +inf).
template <int KP>
__global__ __launch_bounds__(RT_THREADS) void bank_reduce_topk_kernel(const RtPartial* __restrict__ part, int nslabs,
                                                                      int64_t nq, int k, int32_t* __restrict__ idx,
                                                                      float* __restrict__ dist2) {
  const int64_t g = (int64_t)blockIdx.x * RT_THREADS + threadIdx.x;
  if (g >= nq) return;
  float ld[KP];
  int li[KP];
#pragma unroll
  for (int j = 0; j < KP; ++j) {
    const RtPartial c = part[g * KP + j];
    ld[j] = c.d, li[j] = c.idx;
  }
  for (int s = 1; s < nslabs; ++s) {
#pragma unroll
    for (int j = 0; j < KP; ++j) {
      const RtPartial c = part[((int64_t)s * nq + g) * KP + j];
      if (!(c.d < ld[KP - 1])) break;
      list_insert<KP>(ld, li, c.d, c.idx, [](float d, int, float ed, int) { return d < ed; });
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

// ---- blend: gather fp16 value rows (lanes along c), transpose through LDS, mix (lanes along t) ----------------------------
template <bool DENORM>
__global__ __launch_bounds__(RT_THREADS) void bank_blend_kernel(const uint16_t* __restrict__ values, int size, int C,
                                                                const float* x, const int32_t* __restrict__ idx,
                                                                const float* __restrict__ mean, const float* __restrict__ sd,
                                                                float rate, float* y, int T) {
  __shared__ float tile[32][33];
  const int t0 = blockIdx.x * 32, c0 = blockIdx.y * 32, b = blockIdx.z;
  const int lo = threadIdx.x & 31, hi = threadIdx.x >> 5;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int t = t0 + hi + 8 * k;
    if (t < T) {
      int i = idx[(int64_t)b * T + t];
      i = i < 0 ? 0 : (i >= size ? size - 1 : i);
      float v = h2f(values[(int64_t)i * C + c0 + lo]);
      if (DENORM) v = __fadd_rn(__fmul_rn(v, sd[c0 + lo]), mean[c0 + lo]);   // the inverse of channel_affine_kernel
      tile[lo][hi + 8 * k] = v;
    }
  }
  __syncthreads();
  const int t = t0 + lo;
  if (t >= T) return;
  const float keep = 1.f - rate;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t off = ((int64_t)b * C + c0 + hi + 8 * k) * T + t;
    y[off] = __fadd_rn(__fmul_rn(keep, x[off]), __fmul_rn(rate, tile[hi + 8 * k][lo]));   // (1 - r) x + r v, unfused
  }
}

// ---- top-k blend: the weights of a frame once per (block, t), then the gather of bank_blend_kernel over k rows -----------------
// dt_j = max(dist2_j, floor), u_j = (dt_0 / dt_j)^2 (0 where idx_j < 0), w_j = u_j / sum_j u_j, v = sum_j w_j value[idx_j]:
// one division per j, the sum over ascending j, v an fmaf chain over ascending j.  The chain starts from -0, so a single
// term of weight 1 keeps the stored value's bits, the sign of a zero included: k = 1 is bank_blend_kernel bit for bit.
template <bool DENORM>
__global__ __launch_bounds__(RT_THREADS) void bank_blend_topk_kernel(const uint16_t* __restrict__ values, int size, int C,
                                                                     const float* x, const int32_t* __restrict__ idx,
                                                                     const float* __restrict__ dist2, int k, float floor,
                                                                     const float* __restrict__ mean,
                                                                     const float* __restrict__ sd, float rate, float* y,
                                                                     int T) {
  __shared__ float tile[32][33];
  __shared__ float sw[32][RT_MAX_K];
  __shared__ int si[32][RT_MAX_K];
  const int t0 = blockIdx.x * 32, c0 = blockIdx.y * 32, b = blockIdx.z;
  const int lo = threadIdx.x & 31, hi = threadIdx.x >> 5;
  if (threadIdx.x < 32 && t0 + (int)threadIdx.x < T) {
    const int64_t f = ((int64_t)b * T + t0 + threadIdx.x) * k;
    const float d0 = fmaxf(dist2[f], floor);
    float u[RT_MAX_K], S = 0.f;
    int ii[RT_MAX_K];
#pragma unroll
    for (int j = 0; j < RT_MAX_K; ++j) {
      u[j] = 0.f, ii[j] = -1;
      if (j < k) {
        const int i = idx[f + j];
        ii[j] = i >= size ? size - 1 : i;
        if (i >= 0) {
          const float q = __fdiv_rn(d0, fmaxf(dist2[f + j], floor));
          u[j] = __fmul_rn(q, q);
        }
        S = __fadd_rn(S, u[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < RT_MAX_K; ++j) {
      sw[threadIdx.x][j] = S > 0.f ? __fdiv_rn(u[j], S) : 0.f;   // no usable entry at all: v = 0
      si[threadIdx.x][j] = ii[j];
    }
  }
  __syncthreads();
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    const int tl = hi + 8 * kk;
    if (t0 + tl < T) {
      float v = -0.f;
      for (int j = 0; j < k; ++j) {
        const int i = si[tl][j];
        if (i >= 0) v = fmaf(sw[tl][j], h2f(values[(int64_t)i * C + c0 + lo]), v);   // an unused place is not read
      }
      if (DENORM) v = __fadd_rn(__fmul_rn(v, sd[c0 + lo]), mean[c0 + lo]);   // the inverse of channel_affine_kernel
      tile[lo][tl] = v;
    }
  }
  __syncthreads();
  const int t = t0 + lo;
  if (t >= T) return;
  const float keep = 1.f - rate;
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    const int64_t off = ((int64_t)b * C + c0 + hi + 8 * kk) * T + t;
    y[off] = __fadd_rn(__fmul_rn(keep, x[off]), __fmul_rn(rate, tile[hi + 8 * kk][lo]));   // (1 - r) x + r v, unfused
  }
}

size_t search_lds_bytes(int C) {
  const int Cp = (C + RT_KCHUNK - 1) / RT_KCHUNK * RT_KCHUNK;
  return (size_t)(2 * RT_QTILE * (Cp + 8) + RT_KTILE * KROW) * sizeof(uint16_t) + (size_t)9 * RT_QTILE * sizeof(float);
}

template <typename K>
hipError_t allow_lds(K kernel, size_t lds) {
  return hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

}  // namespace

hipError_t bank_pack_launch(const void* src, const void* src2, bool src_fp16, int64_t len, int64_t first, int64_t stride,
                            int count, const float* mean, const float* std, const float* mean2, const float* std2,
                            uint16_t* rows, uint16_t* rows2, int64_t row0, int C, hipStream_t s) {
  if (count <= 0) return hipSuccess;
  const dim3 grid((unsigned)((count + 31) / 32), (unsigned)(C / 32), src2 ? 2u : 1u), block(RT_THREADS);
  if (src_fp16)
    hipLaunchKernelGGL(bank_pack_kernel<_Float16>, grid, block, 0, s, (const _Float16*)src, (const _Float16*)src2, len, first,
                       stride, count, mean, std, mean2, std2, rows, rows2, row0, C);
  else
    hipLaunchKernelGGL(bank_pack_kernel<float>, grid, block, 0, s, (const float*)src, (const float*)src2, len, first, stride,
                       count, mean, std, mean2, std2, rows, rows2, row0, C);
  return hipGetLastError();
}

hipError_t bank_norms_launch(const uint16_t* rows, float* norms, int64_t row0, int count, int C, hipStream_t s) {
  if (count <= 0) return hipSuccess;
  const int per = RT_THREADS / 64;
  hipLaunchKernelGGL(bank_norms_kernel, dim3((unsigned)((count + per - 1) / per)), dim3(RT_THREADS), 0, s, rows, norms, row0,
                     count, C);
  return hipGetLastError();
}

namespace {

// one launcher for every list length: KP = 1 ends in bank_reduce_kernel, the longer lists in bank_reduce_topk_kernel
template <int KP>
hipError_t search_launch(const uint16_t* keys, const float* norms, int size, int C, const float* x, const float* mean,
                         const float* std, int B, int T, int k, int32_t* idx, float* dist2, RtPartial* part, hipStream_t s) {
  static_assert(KROW % 8 == 0 && sizeof(RtPartial) == 8 && 8 * RT_QTILE * KP * sizeof(RtPartial) <= RT_KTILE * KROW * 2,
                "LDS layout of bank_search_kernel: the eight lists of every query fit the key tile");
  static_assert(RT_KTILE * (RT_KCHUNK / 8) == 4 * RT_THREADS && RT_KTILE == 32 * (RT_THREADS / 64) && RT_SLAB % RT_KTILE == 0,
                "tile loader of bank_search_kernel");
  const int64_t nq = (int64_t)B * T;
  const int nslabs = (size + RT_SLAB - 1) / RT_SLAB;
  const size_t lds = search_lds_bytes(C);
  static const hipError_t attr[2] = {allow_lds(bank_search_kernel<false, KP>, search_lds_bytes(RT_MAX_C)),
                                     allow_lds(bank_search_kernel<true, KP>, search_lds_bytes(RT_MAX_C))};
  if (attr[0] != hipSuccess) return attr[0];
  if (attr[1] != hipSuccess) return attr[1];
  const dim3 grid((unsigned)((nq + RT_QTILE - 1) / RT_QTILE), (unsigned)nslabs), block(RT_THREADS);
  if (mean)
    hipLaunchKernelGGL((bank_search_kernel<true, KP>), grid, block, lds, s, keys, norms, size, C, x, mean, std, T, nq, part);
  else
    hipLaunchKernelGGL((bank_search_kernel<false, KP>), grid, block, lds, s, keys, norms, size, C, x, mean, std, T, nq, part);
  const dim3 rgrid((unsigned)((nq + RT_THREADS - 1) / RT_THREADS));
  if constexpr (KP == 1)
    hipLaunchKernelGGL(bank_reduce_kernel, rgrid, block, 0, s, part, nslabs, nq, idx, dist2);
  else
    hipLaunchKernelGGL(bank_reduce_topk_kernel<KP>, rgrid, block, 0, s, part, nslabs, nq, k, idx, dist2);
  return hipGetLastError();
}

}  // namespace

hipError_t bank_search_launch(const uint16_t* keys, const float* norms, int size, int C, const float* x, const float* mean,
                              const float* std, int B, int T, int32_t* idx, float* dist2, RtPartial* part, hipStream_t s) {
  return search_launch<1>(keys, norms, size, C, x, mean, std, B, T, 1, idx, dist2, part, s);
}

hipError_t bank_search_topk_launch(const uint16_t* keys, const float* norms, int size, int C, const float* x,
                                   const float* mean, const float* std, int B, int T, int k, int32_t* idx, float* dist2,
                                   RtPartial* part, hipStream_t s) {
  switch (rt_list_length(k)) {
    case 1: return search_launch<1>(keys, norms, size, C, x, mean, std, B, T, k, idx, dist2, part, s);
    case 2: return search_launch<2>(keys, norms, size, C, x, mean, std, B, T, k, idx, dist2, part, s);
    case 4: return search_launch<4>(keys, norms, size, C, x, mean, std, B, T, k, idx, dist2, part, s);
    default: return search_launch<8>(keys, norms, size, C, x, mean, std, B, T, k, idx, dist2, part, s);
  }
}

hipError_t bank_blend_launch(const uint16_t* values, int size, int C, const float* x, const int32_t* idx, const float* mean,
                             const float* std, float rate, float* y, int B, int T, hipStream_t s) {
  const dim3 grid((unsigned)((T + 31) / 32), (unsigned)(C / 32), (unsigned)B), block(RT_THREADS);
  if (mean)
    hipLaunchKernelGGL(bank_blend_kernel<true>, grid, block, 0, s, values, size, C, x, idx, mean, std, rate, y, T);
  else
    hipLaunchKernelGGL(bank_blend_kernel<false>, grid, block, 0, s, values, size, C, x, idx, mean, std, rate, y, T);
  return hipGetLastError();
}

hipError_t bank_blend_topk_launch(const uint16_t* values, int size, int C, const float* x, const int32_t* idx,
                                  const float* dist2, int k, float floor, const float* mean, const float* std, float rate,
                                  float* y, int B, int T, hipStream_t s) {
  const dim3 grid((unsigned)((T + 31) / 32), (unsigned)(C / 32), (unsigned)B), block(RT_THREADS);
  if (mean)
    hipLaunchKernelGGL(bank_blend_topk_kernel<true>, grid, block, 0, s, values, size, C, x, idx, dist2, k, floor, mean, std,
                       rate, y, T);
  else
    hipLaunchKernelGGL(bank_blend_topk_kernel<false>, grid, block, 0, s, values, size, C, x, idx, dist2, k, floor, mean, std,
                       rate, y, T);
  return hipGetLastError();
}
