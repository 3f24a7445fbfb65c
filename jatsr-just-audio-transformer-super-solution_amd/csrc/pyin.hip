// pYIN (Mauch & Dixon 2014) on YIN's normalised difference: the threshold prior spread over the troughs of a frame, and the
// Viterbi decoding of the pitch track.  The definitions are in include/jat_hip.h and, in fp64, in tests/pyin_ref.py.  fp32 in
// both operand-dtype builds (the parabolic shift and the bin position in fp64), no floating-point atomics, every sum in one
// fixed order.
//
// pyin_observe_kernel.  One block takes one frame at a time.  The frame's candidates y go to LDS; the troughs are compacted
// in lag order (a block scan of per-thread counts); a thread per trough finds the first threshold above its height (q), its
// shift and bin, and claims the bin with an integer LDS max on its position in the list (the largest lag wins).  Then thread
// m - 1 owns threshold m: it walks the list once to count n(m), and once more keeping p(m), the number of troughs under m so
// far, and writes beta_m A[p] / D[n] for PY_CHUNK troughs at a time into an LDS tile; 16 threads per trough add a tile row in a
// fixed order.  The sum over the bins and the logarithms follow.
//
// pyin_viterbi_kernel.  One block per row, one thread per pitch bin s, which owns both states (voiced, unvoiced) of its bin.
// U_h[r] = V_h[r] - logZ[r] of both halves sits interleaved in one LDS array with H entries of -inf either side, so that
// the 2 H + 1 sources of a target are one 8-byte read each, consecutive threads read consecutive entries and the band's
// ends need no branch; the weight of a window position is the same for every thread (a broadcast read).  M_0[s] and M_1[s]
// are found once and used for both targets.  Per frame there are two barriers: one for the block maximum that normalises V
// (wave maxima through LDS), one after U is rewritten in place; every thread has finished reading U before the first, so one
// buffer is enough.  The next frame's log observation is loaded before the window loop.  Back-pointers (16 bits: the source's
// half and its window position) go to scratch.
//
// pyin_trace_kernel.  The same block stages as many frames of back-pointers as fit 48 KiB into LDS, thread 0 follows the
// chain through them, and the block writes state, voiced and f0 of those frames.
#include <float.h>
#include <limits.h>
#include <math.h>

#include "jat_pyin_kernels.h"

#pragma clang fp contract(off)   // every add, subtract and multiply below is rounded once, as the statement has it

extern __shared__ __align__(16) unsigned char py_lds[];

__device__ __forceinline__ bool py_trough(const float* y, int i, int ny) {
  if (i == 0) return y[0] < y[1];
  if (i >= ny - 1) return false;
  return y[i] < y[i - 1] && y[i] <= y[i + 1];
}

__global__ void __launch_bounds__(PY_THREADS)
pyin_observe_kernel(PyinPlan p, const float* __restrict__ cmndf, int frames, int64_t work, float* __restrict__ vp_out,
                    float* __restrict__ lo_out, float* __restrict__ prob_out, int32_t* __restrict__ bin_out,
                    float* __restrict__ obs_out) {
  constexpr int T = PY_THREADS;
  const int tid = threadIdx.x;
  const int ny = p.ny, N = p.n_thresholds, nb = p.n_bins, ntm = p.nt_max;
  const int ntp2 = (ntm + 1) / 2 * 2;
  float* y = (float*)py_lds;                       // [ny]
  float* pr = y + ny;                              // [nt_max] probability per trough
  float* tile = pr + ntm;                          // [PY_CHUNK][PY_TILE_STRIDE]
  int* win = (int*)(tile + PY_CHUNK * PY_TILE_STRIDE);   // [n_bins] list position of the trough that holds the bin, -1: none
  uint16_t* tk = (uint16_t*)(win + nb);            // [nt_max] candidate index of the k-th trough
  uint16_t* tq = tk + ntp2;                        // [nt_max] first threshold above its height, N + 1: none
  uint16_t* tb = tq + ntp2;                        // [nt_max] its bin
  __shared__ float s_val[T];
  __shared__ int s_idx[T], s_cnt[T];

  for (int64_t w = blockIdx.x; w < work; w += gridDim.x) {
    const float* row = cmndf + (size_t)w * (size_t)p.lags + p.min_period;
    __syncthreads();                                          // the frame before is no longer read
    for (int i = tid; i < ny; i += T) y[i] = row[i];
    for (int b = tid; b < nb; b += T) win[b] = -1;
    __syncthreads();

    // troughs in lag order: thread t owns candidates t C .. t C + C - 1
    const int C = (ny + T - 1) / T;
    const int i_lo = tid * C, i_hi = min(ny, i_lo + C);
    int cnt = 0;
    for (int i = i_lo; i < i_hi; ++i) cnt += py_trough(y, i, ny) ? 1 : 0;
    s_cnt[tid] = cnt;
    __syncthreads();
    for (int off = 1; off < T; off <<= 1) {
      const int v = tid >= off ? s_cnt[tid - off] : 0;
      __syncthreads();
      s_cnt[tid] += v;
      __syncthreads();
    }
    const int nt = min(s_cnt[T - 1], ntm);
    int k0 = tid ? s_cnt[tid - 1] : 0;
    for (int i = i_lo; i < i_hi; ++i) {
      if (py_trough(y, i, ny)) {
        if (k0 < ntm) tk[k0] = (uint16_t)i;
        ++k0;
      } else {
        const size_t o = (size_t)w * (size_t)ny + i;
        if (prob_out) prob_out[o] = 0.f;
        if (bin_out) bin_out[o] = -1;
      }
    }
    __syncthreads();

    // per trough: q, shift, bin; the lowest-index trough of minimum height
    float bv = INFINITY;
    int bk = INT_MAX;
    for (int k = tid; k < nt; k += T) {
      const int i = tk[k];
      const float h = y[i];
      const float guess = h * (float)N;                       // a guess; the thresholds themselves decide
      int m = guess < (float)N ? (guess > 0.f ? (int)guess + 1 : 1) : N + 1;
      while (m > 1 && h < p.theta[m - 1]) --m;
      while (m < N + 1 && !(h < p.theta[m])) ++m;
      double shift = 0.0;
      if (i > 0 && i < ny - 1) {
        const double ym = (double)y[i - 1], y0 = (double)h, yp = (double)y[i + 1];
        const double a = (yp + ym) - 2.0 * y0, bb = (yp - ym) / 2.0;
        if (fabs(bb) < fabs(a)) shift = -bb / a;
      }
      const double period = (double)(p.min_period + i) + shift;
      double r = rint(p.bin_scale * log2((p.sr / period) / p.fmin));
      r = r > (double)(nb - 1) ? (double)(nb - 1) : r;
      const int bin = r >= 0.0 ? (int)r : 0;                  // also where r is not a number
      tq[k] = (uint16_t)m, tb[k] = (uint16_t)bin;
      atomicMax(&win[bin], k);
      if (h < bv) bv = h, bk = k;
    }
    s_val[tid] = bv, s_idx[tid] = bk;
    __syncthreads();
    for (int off = T / 2; off > 0; off >>= 1) {
      if (tid < off) {
        const float v = s_val[tid + off];
        const int i = s_idx[tid + off];
        if (v < s_val[tid] || (v == s_val[tid] && i < s_idx[tid])) s_val[tid] = v, s_idx[tid] = i;
      }
      __syncthreads();
    }
    const int gmin = s_idx[0];
    __syncthreads();                                          // s_val is written again below

    // thread m - 1 owns threshold m
    const int m = tid + 1;
    const bool own = m <= N;
    int n_under = 0;
    if (own)
      for (int k = 0; k < nt; ++k) n_under += tq[k] <= m ? 1 : 0;
    const float beta_m = own ? p.beta[m] : 0.f;
    const float inv_d = own && n_under > 0 ? p.invD[n_under] : 0.f;
    int run = 0;                                              // p(m): troughs under threshold m so far
    for (int c0 = 0; c0 < nt; c0 += PY_CHUNK) {
      if (own) {
#pragma unroll 4
        for (int kk = 0; kk < PY_CHUNK; ++kk) {
          const int k = c0 + kk;
          float t = 0.f;
          if (k < nt && tq[k] <= m) {
            t = (beta_m * p.A[run]) * inv_d;
            ++run;
          }
          tile[kk * PY_TILE_STRIDE + tid] = t;
        }
      }
      __syncthreads();
      {
        const int kk = tid >> 4, l = tid & 15, k = c0 + kk;
        float acc = 0.f;
        for (int col = l; col < N; col += 16) acc += tile[kk * PY_TILE_STRIDE + col];
        acc += __shfl_xor(acc, 8, 16);
        acc += __shfl_xor(acc, 4, 16);
        acc += __shfl_xor(acc, 2, 16);
        acc += __shfl_xor(acc, 1, 16);
        if (l == 0 && k < nt) {
          if (k == gmin) acc = acc + p.no_trough_prob * p.cum_beta[tq[k]];
          pr[k] = acc;
        }
      }
      __syncthreads();
    }
    for (int k = tid; k < nt; k += T) {
      const size_t o = (size_t)w * (size_t)ny + tk[k];
      if (prob_out) prob_out[o] = pr[k];
      if (bin_out) bin_out[o] = tb[k];
    }

    // obs, its sum, the log observations
    float part = 0.f;
    float* lo_row = lo_out + (size_t)w * (size_t)(nb + 1);
    for (int b = tid; b < nb; b += T) {
      const int k = win[b];
      const float o = (k >= 0 && k < nt) ? pr[k] : 0.f;
      if (obs_out) obs_out[(size_t)w * (size_t)nb + b] = o;
      lo_row[b] = logf(o + FLT_MIN);
      part += o;
    }
    s_val[tid] = part;
    __syncthreads();
    for (int off = T / 2; off > 0; off >>= 1) {
      if (tid < off) s_val[tid] += s_val[tid + off];
      __syncthreads();
    }
    if (tid == 0) {
      float vp = s_val[0];
      vp = vp < 0.f ? 0.f : (vp > 1.f ? 1.f : vp);
      vp_out[w] = vp;
      lo_row[nb] = logf((1.f - vp) / (float)nb + FLT_MIN);
    }
  }
}

__device__ __forceinline__ float py_wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// blockDim.x = n_bins rounded up to a wave; threads beyond n_bins only take part in the barriers and the maximum
__global__ void __launch_bounds__(PY_MAX_BINS)
pyin_viterbi_kernel(PyinPlan p, const float* __restrict__ log_obs, int frames, uint16_t* __restrict__ back,
                    int32_t* __restrict__ state) {
  const int s = threadIdx.x, nb = p.n_bins, H = p.H, span = 2 * H + 1;
  const int n_waves = blockDim.x >> 6;
  const bool live = s < nb;
  float2* U = (float2*)py_lds;                     // [n_bins + 2 H]: (U_voiced, U_unvoiced) of bin i - H
  float* lwr = (float*)(U + nb + 2 * H);           // [2 H + 1]: the weight of window position j (source s - H + j), logw[2 H - j]
  __shared__ float s_max[PY_MAX_BINS / 64];
  __shared__ int s_arg;
  const float* lo_row = log_obs + (size_t)blockIdx.x * (size_t)frames * (size_t)(nb + 1);
  uint16_t* bp = back + (size_t)blockIdx.x * (size_t)frames * (size_t)(2 * nb);

  for (int i = s; i < nb + 2 * H; i += blockDim.x) U[i] = make_float2(-INFINITY, -INFINITY);
  for (int j = s; j < span; j += blockDim.x) lwr[j] = p.logw[2 * H - j];
  if (s == 0) s_arg = INT_MAX;
  const float logz = live ? p.logZ[s] : 0.f;
  const float lk = p.lk, ls = p.ls;
  float v0 = -INFINITY, v1 = -INFINITY;
  if (live) v0 = lo_row[s] + p.logpi, v1 = lo_row[nb] + p.logpi;
  __syncthreads();
  if (live) U[H + s] = make_float2(v0 - logz, v1 - logz);
  __syncthreads();
  float nx0 = 0.f, nxu = 0.f;
  if (live && frames > 1) nx0 = lo_row[(size_t)(nb + 1) + s], nxu = lo_row[(size_t)(nb + 1) + nb];

  for (int f = 1; f < frames; ++f) {
    const float lo0 = nx0, lou = nxu;
    if (live && f + 1 < frames) {
      const float* nr = lo_row + (size_t)(f + 1) * (size_t)(nb + 1);
      nx0 = nr[s], nxu = nr[nb];
    }
    if (live) {
      float m0 = -INFINITY, m1 = -INFINITY;
      int j0 = H, j1 = H;
      for (int j = 0; j < span; ++j) {
        const float2 u = U[s + j];
        const float wgt = lwr[j];
        const float c0 = u.x + wgt, c1 = u.y + wgt;
        if (c0 > m0) m0 = c0, j0 = j;                         // strict: the lowest source keeps a tie
        if (c1 > m1) m1 = c1, j1 = j;
      }
      const float same0 = m0 + lk, oth0 = m1 + ls, same1 = m1 + lk, oth1 = m0 + ls;
      const bool keep0 = same0 >= oth0;                       // a tie between the halves goes to the voiced source
      const bool keep1 = same1 > oth1;
      v0 = lo0 + (keep0 ? same0 : oth0);
      v1 = lou + (keep1 ? same1 : oth1);
      uint16_t* o = bp + (size_t)f * (size_t)(2 * nb);
      o[s] = (uint16_t)(keep0 ? j0 : (0x8000 | j1));
      o[nb + s] = (uint16_t)(keep1 ? (0x8000 | j1) : j0);
    }
    const float wm = py_wave_max(fmaxf(v0, v1));
    if ((s & 63) == 0) s_max[s >> 6] = wm;
    __syncthreads();                                          // every window read of U lies before this barrier
    float mx = s_max[0];
    for (int q = 1; q < n_waves; ++q) mx = fmaxf(mx, s_max[q]);
    if (live) {
      v0 = v0 - mx, v1 = v1 - mx;
      U[H + s] = make_float2(v0 - logz, v1 - logz);
    }
    __syncthreads();
  }

  // the last state: the lowest-index maximum of V, the voiced half first
  const float wm = py_wave_max(fmaxf(v0, v1));
  __syncthreads();
  if ((s & 63) == 0) s_max[s >> 6] = wm;
  __syncthreads();
  float mx = s_max[0];
  for (int q = 1; q < n_waves; ++q) mx = fmaxf(mx, s_max[q]);
  if (live) {
    const int cand = v0 == mx ? s : (v1 == mx ? nb + s : INT_MAX);
    if (cand != INT_MAX) atomicMin(&s_arg, cand);
  }
  __syncthreads();
  if (s == 0) {
    const int last = s_arg;
    state[(size_t)blockIdx.x * (size_t)frames + (frames - 1)] = (last >= 0 && last < 2 * nb) ? last : 2 * nb - 1;
  }
}

__global__ void __launch_bounds__(256)
pyin_trace_kernel(PyinPlan p, int frames, const uint16_t* __restrict__ back, int32_t* __restrict__ state,
                  float* __restrict__ f0, uint8_t* __restrict__ voiced) {
  const int tid = threadIdx.x, nb = p.n_bins, H = p.H;
  const int FC = pyin_trace_frames(p);
  const int words = nb;                            // 2 n_bins 16-bit back-pointers of one frame are n_bins 32-bit words
  uint32_t* stage = (uint32_t*)py_lds;             // [FC][n_bins]
  __shared__ int s_state[PY_TRACE_MAX];            // the states thread 0 found in the staged frames
  __shared__ int s_cur;
  const size_t base = (size_t)blockIdx.x * (size_t)frames;
  const uint32_t* bp = (const uint32_t*)(back + base * (size_t)(2 * nb));
  if (tid == 0) s_cur = state[base + (frames - 1)];
  __syncthreads();
  if (tid == 0) {
    const int c = s_cur;
    voiced[base + frames - 1] = c < nb ? 1 : 0;
    f0[base + frames - 1] = c < nb ? p.freqs[c] : 0.f;
  }
  // frames f_hi .. f_lo hold the back-pointers that lead to the states of frames f_hi - 1 .. f_lo - 1
  for (int f_hi = frames - 1; f_hi >= 1; f_hi -= FC) {
    const int f_lo = max(1, f_hi - FC + 1), n = f_hi - f_lo + 1;
    const uint32_t* src = bp + (size_t)f_lo * (size_t)words;
    for (int i = tid; i < n * words; i += blockDim.x) stage[i] = src[i];
    __syncthreads();
    if (tid == 0) {
      const uint16_t* e16 = (const uint16_t*)stage;
      int cur = s_cur;
      for (int f = f_hi; f >= f_lo; --f) {
        const int e = e16[(size_t)(f - f_lo) * (size_t)(2 * nb) + cur];
        const int sb = cur < nb ? cur : cur - nb;
        int r = sb - H + (e & 0x7fff);
        r = r < 0 ? 0 : (r > nb - 1 ? nb - 1 : r);            // a decoded chain never leaves the band
        cur = (e >> 15) ? nb + r : r;
        s_state[f - f_lo] = cur;                              // the state of frame f - 1
      }
      s_cur = cur;
    }
    __syncthreads();
    for (int i = tid; i < n; i += blockDim.x) {
      const int c = s_state[i];
      const size_t o = base + (size_t)(f_lo + i - 1);
      state[o] = c;
      voiced[o] = c < nb ? 1 : 0;
      f0[o] = c < nb ? p.freqs[c] : 0.f;
    }
    __syncthreads();
  }
}

hipError_t pyin_observe_launch(const PyinPlan& p, const float* cmndf, int B, int frames, float* voiced_prob, float* log_obs,
                               float* prob, int32_t* bin, float* obs, hipStream_t s) {
  const int64_t work = (int64_t)B * frames;
  const int grid = (int)(work < (1 << 20) ? work : (1 << 20));
  pyin_observe_kernel<<<grid, PY_THREADS, pyin_observe_lds_bytes(p), s>>>(p, cmndf, frames, work, voiced_prob, log_obs, prob,
                                                                          bin, obs);
  return hipGetLastError();
}

hipError_t pyin_forward_launch(const PyinPlan& p, const float* log_obs, int B, int frames, uint16_t* back, int32_t* state,
                               hipStream_t s) {
  pyin_viterbi_kernel<<<B, (p.n_bins + 63) / 64 * 64, pyin_viterbi_lds_bytes(p), s>>>(p, log_obs, frames, back, state);
  return hipGetLastError();
}

hipError_t pyin_trace_launch(const PyinPlan& p, int B, int frames, const uint16_t* back, int32_t* state, float* f0,
                             uint8_t* voiced, hipStream_t s) {
  pyin_trace_kernel<<<B, 256, pyin_trace_lds_bytes(p), s>>>(p, frames, back, state, f0, voiced);
  return hipGetLastError();
}
