// Audio-quality metrics of the reference's calculate_metrics.py (librosa's STFT, log-spectral distance, Slaney mel
// spectrogram in dB) as one STFT-and-reduce pass that never writes a spectrogram to memory, and a small finishing stage.
// Plain fp32 VALU + LDS; the same code in both operand-dtype builds.
//
// STFT pass: a block takes a run of frame groups of one batch row; a group is max(1, 1024 / n_fft) frames transformed
// side by side.  pred and gt of a frame travel as one complex signal z = w (pred + i gt):
//   X_pred[k] = (Z[k] + conj Z[N-k]) / 2,   X_gt[k] = (Z[k] - conj Z[N-k]) / (2i).
// The transform is a Stockham autosort FFT (jat_fft.h, shared with splice.hip), radix 4 with a closing radix-2 pass when
// log2 N is odd, between two LDS buffers.  Every pass reads float2 at unit stride over the lanes (no bank conflict) and
// writes at j0 + r Ns: unit stride from Ns = 16 on; the first pass has no twiddles and runs on the samples as they arrive
// from memory (zeros outside [0, L): the centre padding), each thread storing its four outputs as 32 contiguous bytes.
// Twiddles come from per-pass tables made in fp64 on the host and staged in LDS once per block, indexed [r - 1][k] so that
// lanes read consecutive entries.
// Epilogue per frame: |X|^2 of both signals into LDS; the squared log-magnitude difference summed over bins by a fixed
// shuffle tree in fp64 (lsd_frames); the sparse mel bands, each eight lanes' strided fp32 sums and a fixed tree.  Every
// output is summed in an order that depends on neither the batch nor the block it falls in, maxima are exact, and there are
// no atomics: the same bits from run to run and for a row alone or in a batch.  The two signals of a frame share the
// rounding of one transform: a bin is accurate to about 1e-7 of the frame's energy in BOTH signals, so a signal far below
// its partner (more than about 120 dB) reads as the partner's rounding noise; a frame of exact zeros is kept exactly zero.
#include "jat_fft.h"

namespace {

__global__ void __launch_bounds__(MT_THREADS)
stft_metrics_kernel(MetricsPlan p, MetricsTables t, const float* __restrict__ pred, const float* __restrict__ gt, int L,
                    int frames, int gpb, float* __restrict__ mel_pow, float* __restrict__ block_max,
                    float* __restrict__ lsd_frames, float2* __restrict__ Xp, float2* __restrict__ Xg) {
  extern __shared__ __align__(16) float2 lds[];
  const int N = p.n_fft, G = p.group, bins = p.bins, tid = threadIdx.x, b = blockIdx.y;
  float2* buf0 = lds;
  float2* buf1 = lds + G * N;
  float2* tw = buf1 + G * N;
  double* red = (double*)(tw + ((p.n_tw + 1) & ~1));   // [4] wave sums of the LSD reduction
  float* mxs = (float*)(red + 4);                       // [2][4] wave maxima
  int* live = (int*)(mxs + 8);                          // [G][2] does the frame hold a non-zero sample of pred / of gt
  for (int i = tid; i < p.n_tw; i += MT_THREADS) tw[i] = t.tw[i];
  if (tid < 2 * G) live[tid] = 0;
  __syncthreads();

  const float* pr = pred + (int64_t)b * L;
  const float* gr = gt + (int64_t)b * L;
  const int tpf = MT_THREADS / G;            // threads that share one frame in the epilogue (16..256)
  const int ge = tid / tpf, l = tid - ge * tpf;
  const int q = N >> 2, lq = 31 - __clz(q);
  float mxp = 0.f, mxg = 0.f;                // mel powers are >= 0

  for (int grp = 0; grp < gpb; ++grp) {
    const int fbase = (blockIdx.x * gpb + grp) * G;
    if (fbase >= frames) break;              // the same for every thread of the block
    // pass 0 (Ns = 1, no twiddles) on the windowed samples as they are loaded
    for (int jj = tid; jj < G * q; jj += MT_THREADS) {
      const int g = jj >> lq, j = jj & (q - 1), f = fbase + g;
      float2 v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = j + r * q;
        const int64_t s = (int64_t)f * p.hop + i - (N >> 1);
        const bool in = f < frames && s >= 0 && s < L;
        const float w = t.window[i];
        v[r] = make_float2(in ? w * pr[s] : 0.f, in ? w * gr[s] : 0.f);
      }
      // a frame of zeros has a zero spectrum: kept exact, not left to the rounding of the partner's transform
      if (v[0].x != 0.f || v[1].x != 0.f || v[2].x != 0.f || v[3].x != 0.f) live[2 * g] = 1;
      if (v[0].y != 0.f || v[1].y != 0.f || v[2].y != 0.f || v[3].y != 0.f) live[2 * g + 1] = 1;
      fft_first_pass(v, buf0 + g * N, j);
    }
    __syncthreads();
    float2* dst;
    float2* src = fft_later_passes(p, tw, buf0, buf1, G, tid, &dst);

    // epilogue, part 1: split Z into the two spectra; powers into LDS (the buffer the last pass read from)
    const int f = fbase + ge;
    const bool valid = f < frames;
    const float2* Z = src + ge * N;
    float* pwp = (float*)(dst + ge * N);     // [bins] |X_pred|^2, then [bins] |X_gt|^2: N + 2 <= 2 N floats
    float* pwg = pwp + bins;
    double acc = 0.0;
    // the band weights of this group travel to LDS behind the bin loop: into the half of frame 0's power buffer that the
    // powers leave free, N - 2 floats (a bin lies under at most two triangles and the two edge bins under none)
    const bool stage_w = mel_pow != nullptr;
    float wr[MT_W_PER_THREAD];
    if (stage_w) {
#pragma unroll
      for (int u = 0; u < MT_W_PER_THREAD; ++u) {
        const int i = tid + u * MT_THREADS;
        wr[u] = i < p.nnz ? t.band_w[i] : 0.f;
      }
    }
    if (valid) {
      const bool lp = live[2 * ge] != 0, lg = live[2 * ge + 1] != 0;
      for (int k = l; k < bins; k += tpf) {
        const float2 a = Z[k], c = Z[(N - k) & (N - 1)];
        const float2 xp = lp ? make_float2(0.5f * (a.x + c.x), 0.5f * (a.y - c.y)) : make_float2(0.f, 0.f);
        const float2 xg = lg ? make_float2(0.5f * (a.y + c.y), -0.5f * (a.x - c.x)) : make_float2(0.f, 0.f);
        const float pp = xp.x * xp.x + xp.y * xp.y, pg = xg.x * xg.x + xg.y * xg.y;
        pwp[k] = pp;
        pwg[k] = pg;
        if (lsd_frames) {
          // log10 max(|X|, 1e-8) = log10 max(|X|^2, 1e-16) / 2
          const float d = 0.5f * (log10f(fmaxf(pp, 1e-16f)) - log10f(fmaxf(pg, 1e-16f)));
          acc += (double)d * (double)d;
        }
        if (Xp) Xp[((int64_t)b * bins + k) * frames + f] = xp;
        if (Xg) Xg[((int64_t)b * bins + k) * frames + f] = xg;
      }
    }
    float* wl = (float*)dst + N + 2;
    if (stage_w) {
#pragma unroll
      for (int u = 0; u < MT_W_PER_THREAD; ++u) {
        const int i = tid + u * MT_THREADS;
        if (i < p.nnz) wl[i] = wr[u];
      }
    }
    if (lsd_frames) {
      const int seg = tpf < 64 ? tpf : 64;
      for (int o = seg >> 1; o > 0; o >>= 1) acc += __shfl_down(acc, o, seg);
      if (tpf > 64 && (tid & 63) == 0) red[tid >> 6] = acc;
    }
    __syncthreads();
    // part 2: lsd_frames and the mel bands
    if (l < 2) live[2 * ge + l] = 0;         // read in part 1 only; the next group sets it after the closing barrier
    if (valid) {
      if (lsd_frames && l == 0) {
        if (tpf > 64) {
          const int wpf = tpf >> 6;
          acc = red[ge * wpf];
          for (int w = 1; w < wpf; ++w) acc += red[ge * wpf + w];
        }
        lsd_frames[(int64_t)b * frames + f] = sqrtf((float)(acc / (double)bins));
      }
      if (mel_pow) {
        float* mp = mel_pow + ((int64_t)b * 2 * frames + f) * p.n_mels;
        float* mg = mp + (int64_t)frames * p.n_mels;
        // eight lanes share a band: lane s adds the terms s, s + 8, ... in ascending order, then a fixed three-step tree
        const int sub = l & 7;
        for (int m = l >> 3; m < p.n_mels; m += tpf >> 3) {
          const int first = t.band_first[m], cnt = t.band_count[m];
          const float* w = wl + t.band_off[m];
          float sp = 0.f, sg = 0.f;
          for (int i = sub; i < cnt; i += 8) {
            const float wi = w[i];
            sp = fmaf(wi, pwp[first + i], sp);
            sg = fmaf(wi, pwg[first + i], sg);
          }
          for (int o = 4; o > 0; o >>= 1) {
            sp += __shfl_down(sp, o, 8);
            sg += __shfl_down(sg, o, 8);
          }
          if (sub == 0) {
            mp[m] = sp;
            mg[m] = sg;
            mxp = fmaxf(mxp, sp);
            mxg = fmaxf(mxg, sg);
          }
        }
      }
    }
    __syncthreads();                         // the next group overwrites both buffers
  }

  if (block_max) {
    for (int o = 32; o > 0; o >>= 1) {
      mxp = fmaxf(mxp, __shfl_down(mxp, o, 64));
      mxg = fmaxf(mxg, __shfl_down(mxg, o, 64));
    }
    if ((tid & 63) == 0) {
      mxs[tid >> 6] = mxp;
      mxs[4 + (tid >> 6)] = mxg;
    }
    __syncthreads();
    if (tid < 2) {
      const float* m = mxs + 4 * tid;
      block_max[((int64_t)b * 2 + tid) * gridDim.x + blockIdx.x] = fmaxf(fmaxf(m[0], m[1]), fmaxf(m[2], m[3]));
    }
  }
}

// 10 log10 max(1e-10, s), and its level under a reference floored at -80 dB.  The product is rounded on its own (no fused
// multiply-subtract with the reference level), so the loudest element is exactly 0 dB.
__device__ __forceinline__ float power_db(float s) {
#pragma clang fp contract(off)
  return 10.f * log10f(fmaxf(1e-10f, s));
}
__device__ __forceinline__ float level_db(float s, float ref_db) {
#pragma clang fp contract(off)
  const float ls = 10.f * log10f(fmaxf(1e-10f, s));
  return fmaxf(ls - ref_db, -80.f);
}

// Stage 1 of the finish: block (s, b) converts slice s of row b's mel powers to dB against the row's maxima, floors them at
// -80 dB, and sums |a - b|, (a - b)^2 and its slice of lsd_frames in fp64: thread-strided partial sums, then a fixed tree.
__global__ void __launch_bounds__(256)
metrics_partial_kernel(const float* __restrict__ mel_pow, const float* __restrict__ block_max, int nbx,
                       const float* __restrict__ lsd_frames, int frames, int n_mels, double* __restrict__ partial,
                       float* __restrict__ pred_db, float* __restrict__ gt_db) {
  __shared__ double r1[256], r2[256], r3[256];
  __shared__ float mx[2][256];
  const int s = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  double s1 = 0.0, s2 = 0.0, s3 = 0.0;
  if (mel_pow) {
    float mp = 0.f, mg = 0.f;
    for (int i = tid; i < nbx; i += 256) {
      mp = fmaxf(mp, block_max[(int64_t)b * 2 * nbx + i]);
      mg = fmaxf(mg, block_max[((int64_t)b * 2 + 1) * nbx + i]);
    }
    mx[0][tid] = mp;
    mx[1][tid] = mg;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (tid < w) {
        mx[0][tid] = fmaxf(mx[0][tid], mx[0][tid + w]);
        mx[1][tid] = fmaxf(mx[1][tid], mx[1][tid + w]);
      }
      __syncthreads();
    }
    const float refp = power_db(mx[0][0]), refg = power_db(mx[1][0]);
    const int64_t total = (int64_t)frames * n_mels;
    const int64_t chunk = (total + MT_SLICES - 1) / MT_SLICES;
    const int64_t e0 = s * chunk, e1 = min(total, e0 + chunk);
    const float* pp = mel_pow + (int64_t)b * 2 * total;
    const float* pg = pp + total;
    for (int64_t e = e0 + tid; e < e1; e += 256) {
      const float a = level_db(pp[e], refp), c = level_db(pg[e], refg);
      if (pred_db) {
        const int64_t f = e / n_mels, m = e - f * n_mels;
        pred_db[((int64_t)b * n_mels + m) * frames + f] = a;
        gt_db[((int64_t)b * n_mels + m) * frames + f] = c;
      }
      const double d = (double)a - (double)c;
      s1 += fabs(d);
      s2 += d * d;
    }
  }
  if (lsd_frames) {
    const int chunk = (frames + MT_SLICES - 1) / MT_SLICES;
    const int f0 = s * chunk, f1 = min(frames, f0 + chunk);
    for (int f = f0 + tid; f < f1; f += 256) s3 += (double)lsd_frames[(int64_t)b * frames + f];
  }
  r1[tid] = s1;
  r2[tid] = s2;
  r3[tid] = s3;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) {
      r1[tid] += r1[tid + w];
      r2[tid] += r2[tid + w];
      r3[tid] += r3[tid + w];
    }
    __syncthreads();
  }
  if (tid == 0) {
    double* o = partial + ((int64_t)b * MT_SLICES + s) * 3;
    o[0] = r1[0];
    o[1] = r2[0];
    o[2] = r3[0];
  }
}

// Stage 2: one thread per row adds its slices in order.  out [B, 3]: lsd_db, mel_l1, mel_l2.
__global__ void __launch_bounds__(256)
metrics_final_kernel(const double* __restrict__ partial, int B, int frames, int n_mels, double* __restrict__ out) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  double s1 = 0.0, s2 = 0.0, s3 = 0.0;
  for (int s = 0; s < MT_SLICES; ++s) {
    const double* q = partial + ((int64_t)b * MT_SLICES + s) * 3;
    s1 += q[0];
    s2 += q[1];
    s3 += q[2];
  }
  const double n = (double)frames * (double)(n_mels > 0 ? n_mels : 1);
  out[b * 3] = 20.0 * s3 / (double)frames;
  out[b * 3 + 1] = s1 / n;
  out[b * 3 + 2] = sqrt(s2 / n);
}

}  // namespace

int metrics_groups_per_block(const MetricsPlan& p, int B, int frames) {
  // as few groups per block as keep the launch within the blocks the chip holds at once: a second, nearly empty round of
  // blocks would cost as much as the first
  const int64_t groups = ((int64_t)frames + p.group - 1) / p.group * B;
  int64_t g = (groups + p.slots - 1) / p.slots;
  return (int)(g < 1 ? 1 : (g > 64 ? 64 : g));
}

hipError_t metrics_blocks_per_cu(const MetricsPlan& p, int* blocks) {
  const size_t lds = metrics_lds_bytes(p);
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)stft_metrics_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, (const void*)stft_metrics_kernel, MT_THREADS, lds);
}

size_t metrics_lds_bytes(const MetricsPlan& p) {
  return ((size_t)2 * p.group * p.n_fft + ((p.n_tw + 1) & ~1)) * sizeof(float2) + 4 * sizeof(double) + 8 * sizeof(float) + 32 * sizeof(int);
}

hipError_t metrics_stft_launch(const MetricsPlan& p, const MetricsTables& t, const float* pred, const float* gt, int B, int L,
                               int frames, float* mel_pow, float* block_max, float* lsd_frames, float2* Xp, float2* Xg,
                               hipStream_t s) {
  const int gpb = metrics_groups_per_block(p, B, frames);
  const dim3 grid(metrics_blocks_per_row(p, B, frames), B);
  const size_t lds = metrics_lds_bytes(p);
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)stft_metrics_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  stft_metrics_kernel<<<grid, MT_THREADS, lds, s>>>(p, t, pred, gt, L, frames, gpb, mel_pow, block_max, lsd_frames, Xp, Xg);
  return hipGetLastError();
}

hipError_t metrics_finish_launch(const MetricsPlan& p, const float* mel_pow, const float* block_max, int blocks_per_row,
                                 const float* lsd_frames, int B, int frames, double* partial, double* out, float* pred_db,
                                 float* gt_db, hipStream_t s) {
  metrics_partial_kernel<<<dim3(MT_SLICES, B), 256, 0, s>>>(mel_pow, block_max, blocks_per_row, lsd_frames, frames, p.n_mels,
                                                            partial, pred_db, gt_db);
  metrics_final_kernel<<<(B + 255) / 256, 256, 0, s>>>(partial, B, frames, p.n_mels, out);
  return hipGetLastError();
}
