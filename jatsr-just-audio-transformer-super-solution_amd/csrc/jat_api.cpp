// C-ABI host side of libjat_hip.so (declarations and contracts: include/jat_hip.h).
// Owns the packed weights, lays out the caller's workspace, sequences the gfx950 kernels of one DiT forward
// on the caller's stream, and captures the 50-step CFG sampler into a hipGraph.  No arithmetic happens here.
#include "../../include/jat_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "jat_internal.h"
#include "jat_dtype.h"
#include "gemm_plan.h"
#include "gemm_variants.h"

static thread_local char g_err[512] = "";
int jat_fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

// workspace carve-up for a forward over `B` batch rows of `ntok` tokens
struct Workspace {
  bf16_t *a_patch, *h_patch, *xn, *xlo, *q, *k, *vt, *ao, *hm, *t_silu;
  float *x, *mod, *e_sin, *t_h, *t_emb, *part;
  float* kpart;   // split-K partials when M is too small to fill the chip (nullptr for large M: split_ws_slices, gemm_plan.h)
  const int* lens = nullptr;   // sampler: per-batch-row key counts (tokens) for the attention kernel, or nullptr
  const int* tvalid = nullptr; // sampler: valid frames per source row (patchify reads zeros beyond them), or nullptr
  int npad;
  size_t vt_bytes, total;
};

static Workspace carve(const jat_model* m, int B, int ntok, char* base) {
  Workspace w;
  size_t off = 0;
  const size_t M = (size_t)B * ntok;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += align_up(bytes, 256);
    return p;
  };
  w.npad = (int)align_up((size_t)ntok, 64);
  w.a_patch = (bf16_t*)take(M * m->Kp * 2);
  w.h_patch = (bf16_t*)take(M * m->bott * 2);
  w.x = (float*)take(M * m->D * 4);
  w.xn = (bf16_t*)take(M * m->D * 2);
  w.xlo = (bf16_t*)take(M * m->D * 2);   // lo plane of the split residual stream (sampler with folded norms; hi = xn)
  w.q = (bf16_t*)take(M * m->D * 2);
  w.k = (bf16_t*)take(M * m->kvD * 2);
  w.vt_bytes = (size_t)B * m->Hkv * HEAD_DIM * w.npad * 2;
  w.vt = (bf16_t*)take(w.vt_bytes);
  w.ao = (bf16_t*)take(M * m->D * 2);
  w.hm = (bf16_t*)take(M * m->mlp * 2);
  w.mod = (float*)take((size_t)B * m->depth * 6 * m->D * 4);
  w.e_sin = (float*)take((size_t)B * m->D * 4);
  w.t_h = (float*)take((size_t)B * m->D * 4);
  w.t_emb = (float*)take((size_t)B * m->D * 4);
  w.t_silu = (bf16_t*)take((size_t)B * m->D * 2);
  w.part = (float*)take(M * 32 * 4);  // row partial sums of x^2 (norm folding), <= 32 wave column tiles
  w.kpart = split_ws_slices(M) ? (float*)take((size_t)split_ws_slices(M) * M * (m->D + 2 * m->kvD) * 4) : nullptr;   // widest user: the QKV GEMM
  w.total = off;
  return w;
}

extern "C" const char* jat_last_error(void) { return g_err; }
extern "C" int jat_version(void) { return 2; }
extern "C" int jat_operand_dtype(void) { return JAT_OPERAND_DTYPE; }   // 0 bf16, 1 fp16 (jat_dtype.h)

// ---------------------------------------------------------------------------------------------------------
// model
// ---------------------------------------------------------------------------------------------------------
extern "C" int jat_model_create(const jat_config* c, jat_model** out) {
  if (!c || !out) return fail(JAT_E_INVALID, "null argument");
  // same checks as the reference constructor asserts (jat_audiosr_v3.py:119-120) plus kernel limits
  if (c->num_q_heads <= 0 || c->hidden_size % c->num_q_heads != 0)
    return fail(JAT_E_INVALID, "hidden_size must be divisible by num_q_heads");
  if (c->num_kv_heads <= 0 || c->num_q_heads % c->num_kv_heads != 0)
    return fail(JAT_E_INVALID, "num_q_heads must be divisible by num_kv_heads");
  if (c->hidden_size / c->num_q_heads != HEAD_DIM) return fail(JAT_E_INVALID, "head_dim must be 64");
  if (c->patch_len != 4) return fail(JAT_E_INVALID, "patch_len must be 4");
  if (c->hidden_size % 256 != 0 || c->hidden_size > 2048)
    return fail(JAT_E_INVALID, "hidden_size must be a multiple of 256, <= 2048");
  if (c->bottleneck_dim % 128 != 0 || c->mlp_hidden % 128 != 0)
    return fail(JAT_E_INVALID, "bottleneck_dim and mlp_hidden must be multiples of 128");
  if (c->input_channels % 32 != 0 || c->cond_channels % 32 != 0 || c->input_channels <= 0 || c->cond_channels <= 0)
    return fail(JAT_E_INVALID, "channel counts must be positive multiples of 32");
  if (c->depth <= 0) return fail(JAT_E_INVALID, "depth must be positive");
  if (c->norm_mode != JAT_NORM_RMS_W && c->norm_mode != JAT_NORM_LN_NOAFFINE)
    return fail(JAT_E_INVALID, "unknown norm_mode");
  jat_model* m = new jat_model();
  m->cfg = *c;
  m->D = c->hidden_size; m->depth = c->depth; m->Hq = c->num_q_heads; m->Hkv = c->num_kv_heads;
  m->kvD = m->Hkv * HEAD_DIM; m->mlp = c->mlp_hidden; m->bott = c->bottleneck_dim;
  m->Cin = c->input_channels; m->Cc = c->cond_channels; m->P = 4;
  m->Kp = m->P * (m->Cin + m->Cc); m->Fout = m->P * m->Cin;
  auto env_int = [](const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; };
  m->sw.fuse_qkv_attn = env_int("JAT_FUSE_QKV_ATTN", 1); m->sw.qkv_split = env_int("JAT_QKV_SPLIT", 1);
  m->sw.fuse_finish = env_int("JAT_FUSE_FINISH", 1); m->sw.fold_norm = env_int("JAT_FOLD_NORM", 1);
  m->sw.split_patch = env_int("JAT_SPLIT_PATCH", 1); m->sw.fuse_euler = env_int("JAT_FUSE_EULER", 1);
  m->sw.fold_cap_mb = env_int("JAT_FOLD_CAP_MB", 0); m->sw.patch_split = env_int("JAT_PATCH_SPLIT", 1);
  if (const char* v = getenv("JAT_GEMM_VARIANT"))
    for (int i = 0; i < 5; ++i) m->variants[i] = atoi(v);
  if (const char* v = getenv("JAT_GEMM_VARIANTS")) {  // "qkv,out,fc1,fc2,other"
    int x[5];
    if (sscanf(v, "%d,%d,%d,%d,%d", &x[0], &x[1], &x[2], &x[3], &x[4]) == 5)
      for (int i = 0; i < 5; ++i) m->variants[i] = x[i];
  }
  jat_describe_params(m);
  *out = m;
  return JAT_OK;
}

extern "C" int jat_model_set_switch(jat_model* m, const char* name, int32_t value) {
  if (!m || !name) return fail(JAT_E_INVALID, "null argument");
  const std::string n(name);
  int* slot = n == "fuse_qkv_attn" ? &m->sw.fuse_qkv_attn : n == "qkv_split" ? &m->sw.qkv_split : n == "fuse_finish" ? &m->sw.fuse_finish
            : n == "fold_norm" ? &m->sw.fold_norm : n == "split_patch" ? &m->sw.split_patch
            : n == "fold_cap_mb" ? &m->sw.fold_cap_mb : n == "patch_split" ? &m->sw.patch_split
            : n == "fuse_euler" ? &m->sw.fuse_euler : nullptr;
  if (!slot) return fail(JAT_E_INVALID, "unknown switch '%s'", name);
  *slot = value;
  return JAT_OK;
}

extern "C" void jat_model_destroy(jat_model* m) {
  if (!m) return;
  for (hipEvent_t e : m->prof.ev) (void)hipEventDestroy(e);
  if (m->blob) (void)hipFree(m->blob);
  delete m;
}

extern "C" int jat_model_load_weights(jat_model* m, const jat_tensor_ref* named, int32_t n, void* stream_) {
  if (!m || !named) return fail(JAT_E_INVALID, "null argument");
  return jat_pack_weights(m, named, n, (hipStream_t)stream_);
}

int jat_pack_weights(jat_model* m, const jat_tensor_ref* named, int32_t n, hipStream_t s) {
  std::unordered_map<std::string, const jat_tensor_ref*> by_name;
  for (int i = 0; i < n; ++i) by_name[named[i].name] = &named[i];
  // every parameter present and of the expected size, before anything is allocated or converted
  std::vector<const float*> src(m->params.size(), nullptr);
  for (size_t i = 0; i < m->params.size(); ++i) {
    const ParamDesc& e = m->params[i];
    if (!m->has(e)) continue;
    auto it = by_name.find(e.name);
    if (it == by_name.end()) return fail(JAT_E_STATE, "missing parameter '%s'", e.name.c_str());
    if (it->second->numel != e.numel())
      return fail(JAT_E_INVALID, "parameter '%s' has %lld elements, expected %lld", e.name.c_str(),
                  (long long)it->second->numel, (long long)e.numel());
    src[i] = it->second->data;
  }
  auto source = [&](int id, int block) -> const float* {
    for (size_t i = 0; i < src.size(); ++i)
      if (m->params[i].id == id && m->params[i].block == block) return src[i];
    return nullptr;
  };
  if (!m->blob) {
    HIPCHK(hipMalloc((void**)&m->blob, m->blob_bytes));
    for (const BlobSlot& t : m->slots) {
      if (t.h) *t.h = (bf16_t*)(m->blob + t.off);
      else *t.f = (float*)(m->blob + t.off);
    }
  }
  m->fold_cache.clear();   // folded tables belong to the previous weights (samplers that still hold one keep it alive)
  m->fold_src_ok = false;

  // ---- the parameters: copy / convert each to its operand copy ----
  for (size_t i = 0; i < m->params.size(); ++i) {
    const ParamDesc& e = m->params[i];
    if (e.form == F_BF16_ROPE) {
      KCHK(launch_cast_bf16_rope_rows(src[i], m->at<bf16_t>(e), e.rows, e.cols, s));
    } else if (e.form == F_BF16) {
      KCHK(launch_cast_bf16(src[i], m->at<bf16_t>(e), e.numel(), s));
    } else if (m->has(e)) {
      HIPCHK(hipMemcpyAsync(m->at<float>(e), src[i], e.numel() * 4, hipMemcpyDeviceToDevice, s));
    }
  }

  // ---- what is not a parameter: constant-ones norm weights (LayerNorm models), group-major QKV (group5), fold sources (keep32) ----
  const int D = m->D, kvD = m->kvD;
  const bool group5 = m->layers[0].wqkv_g != nullptr, keep32 = m->wfinal32 != nullptr;   // as laid out by jat_describe_params
  for (const ParamDesc& e : m->params) {
    if (m->has(e)) continue;
    const std::vector<float> ones(e.numel(), 1.0f);
    HIPCHK(hipMemcpyAsync(m->at<float>(e), ones.data(), e.numel() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
  }
  for (int l = 0; l < m->depth; ++l) {
    const LayerW& L = m->layers[l];
    const float *wq = source(P_Q, l), *wk = source(P_K, l), *wv = source(P_V, l);
    if (group5) {     // group-major copy: per KV head g: 5 q heads, its k head, its v head
      for (int g = 0; g < m->Hkv; ++g) {
        bf16_t* dst = L.wqkv_g + (int64_t)g * 448 * D;
        KCHK(launch_cast_bf16_rope_rows(wq + (int64_t)g * 320 * D, dst, 320, D, s));
        KCHK(launch_cast_bf16_rope_rows(wk + (int64_t)g * 64 * D, dst + (int64_t)320 * D, 64, D, s));
        KCHK(launch_cast_bf16(wv + (int64_t)g * 64 * D, dst + (int64_t)384 * D, (int64_t)64 * D, s));
      }
    }
    if (keep32) {     // fold sources: refreshed on a full load only (a training re-pack leaves them stale)
      HIPCHK(hipMemcpyAsync(L.q32, wq, (size_t)D * D * 4, hipMemcpyDeviceToDevice, s));
      HIPCHK(hipMemcpyAsync(L.k32, wk, (size_t)kvD * D * 4, hipMemcpyDeviceToDevice, s));
      HIPCHK(hipMemcpyAsync(L.v32, wv, (size_t)kvD * D * 4, hipMemcpyDeviceToDevice, s));
      HIPCHK(hipMemcpyAsync(L.w132, source(P_W1, l), (size_t)m->mlp * D * 4, hipMemcpyDeviceToDevice, s));
    }
  }
  if (keep32) HIPCHK(hipMemcpyAsync(m->wfinal32, source(P_WF, m->depth), (size_t)m->Fout * D * 4, hipMemcpyDeviceToDevice, s));
  // RoPE tables in fp32 exactly as RoPE.__init__ builds them (jat_audiosr_v3.py:77-85); only the first half
  // of `emb = cat([freqs, freqs])` is distinct.
  std::vector<float> hc((size_t)MAX_LEN * 32), hs((size_t)MAX_LEN * 32), hf(32);
  for (int i = 0; i < 32; ++i) {
    const float inv_freq = 1.0f / powf(10000.0f, (float)(2 * i) / 64.0f);
    hf[i] = inv_freq;
    for (int pos = 0; pos < MAX_LEN; ++pos) {
      const float a = (float)pos * inv_freq;
      hc[(size_t)pos * 32 + i] = cosf(a);
      hs[(size_t)pos * 32 + i] = sinf(a);
    }
  }
  HIPCHK(hipMemcpyAsync(m->rope_cos, hc.data(), hc.size() * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(m->rope_sin, hs.data(), hs.size() * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(m->rope_invf, hf.data(), hf.size() * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));
  m->group_copy_stale = false;
  m->fold_src_ok = keep32;
  m->loaded = true;
  return JAT_OK;
}

extern "C" int jat_model_workspace_bytes(const jat_model* m, int32_t B, int32_t T, size_t* out) {
  if (!m || !out || B <= 0 || T <= 0) return fail(JAT_E_INVALID, "bad argument");
  const int ntok = (T + 3) / 4;
  *out = carve(m, B, ntok, nullptr).total;
  return JAT_OK;
}

// ---------------------------------------------------------------------------------------------------------
// forward pieces
// ---------------------------------------------------------------------------------------------------------

// plan == nullptr: a plain GEMM of the call site (plan_gemm), in extra.ksplit slices if the caller set them up itself (the
// training step's dW GEMMs); else what one of the per-decision functions of gemm_plan.h returned
int jat_gemm(const jat_model* m, int site, const bf16_t* A, int64_t lda, const bf16_t* W, int64_t ldw, int M, int N,
             int K, int epi, GemmArgs extra, hipStream_t s, const GemmPlan* plan) {
  GemmArgs a = extra;
  a.A = A; a.lda = lda; a.W = W; a.ldw = ldw; a.M = M; a.N = N; a.K = K;
  const GemmPlan p = plan ? *plan : plan_gemm(m, site, M, N, a.ksplit, a.fold_out || a.rs_part);
  if (p.ksplit > 1) { a.ksplit = p.ksplit; a.K = K / p.ksplit; }   // per-slice depth; the kernel shifts A / W / out by blockIdx.y
  const GemmVariant* t = gemm_variant(p.variant);   // nullptr (a pinned id that is not live): launch_gemm rejects it
  if (a.fold_out) { a.fold_np = t ? N / t->wave_n() : 0; m->last_fold_np = a.fold_np; }
  if (a.rs_part) a.rs_np = m->last_fold_np;
  // measurement aid (bench.py roofline leg): bracket the launches of one call site with HIP events on the
  // launch stream.  Never active during graph capture (the bench enables it around eager forwards only).
  const bool timed = m->prof.site == site && m->prof.n < (int)m->prof.ev.size() / 2;
  if (timed) { m->prof.stream = s; (void)hipEventRecord(m->prof.ev[2 * m->prof.n], s); }
  hipError_t e = launch_gemm(a, epi, p.variant, s);
  if (timed) {
    (void)hipEventRecord(m->prof.ev[2 * m->prof.n + 1], s);
    m->prof.flops += 2.0 * M * N * K;
    m->prof.variant = p.variant;
    ++m->prof.n;
  }
  if (e != hipSuccess) return fail(JAT_E_HIP, "gemm launch (M=%d N=%d K=%d epi=%d): %s", M, N, K, epi, hipGetErrorString(e));
  return JAT_OK;
}

// t [B] -> t_emb [B,D] fp32 (+ bf16 silu(t_emb))  (t_embedder, jat_audiosr_v3.py:364-369)
static int time_path(const jat_model* m, const Workspace& w, const float* t, int B, hipStream_t s) {
  KCHK(launch_time_sinusoid(t, w.e_sin, B, m->D, s));
  KCHK(launch_linear_f32(w.e_sin, m->te_w1, m->te_b1, w.t_h, nullptr, B, m->D, m->D, 1, s));
  KCHK(launch_linear_f32(w.t_h, m->te_w2, m->te_b2, w.t_emb, w.t_silu, B, m->D, m->D, 0, s));
  return JAT_OK;
}
// silu(t_emb) bf16 [B,D] -> mod [B, nlayers*6D] for layers [l0, l0+nl)  (adaLN_modulation, :275-278)
static int adaln_path(const jat_model* m, const bf16_t* t_silu, float* mod, int B, int l0, int nl, hipStream_t s) {
  GemmArgs e{};
  e.out = mod; e.ldo = (int64_t)nl * 6 * m->D; e.bias = m->bada + (int64_t)l0 * 6 * m->D; e.ntok = 1;
  return jat_gemm(m, G_OTHER, t_silu, m->D, m->wada + (int64_t)l0 * 6 * m->D * m->D, m->D, B, nl * 6 * m->D, m->D, EPI_F32, e, s);
}

// Norm folding (sampler path, RMSNorm only): this step's slice of the FoldTable (jat_internal.h); layer offsets are applied
// in run_block.  wqkv_g != nullptr selects the fused QKV+attention kernel (group-major weights), else wqkv_i.
struct Fold {
  const bf16_t *wqkv_g, *wqkv_i, *w1, *wfinal;
  const float *bq_g, *bq_i, *bf;
};

static constexpr float kAttnScaleLog2e = 0.125f * 1.4426950408889634f;   // (1 / sqrt(64)) * log2(e)
static GemmArgs qkv_rope_args(const jat_model* m, const Workspace& w, int ntok) {
  GemmArgs e{};
  e.out = w.q; e.k_out = w.k; e.vt_out = w.vt; e.D = m->D; e.kvD = m->kvD; e.npad = w.npad; e.ntok = ntok;
  e.rope_cos = m->rope_cos; e.rope_sin = m->rope_sin; e.rope_inv_freq = m->rope_invf;
  return e;
}
static AttnArgs attn_args(const jat_model* m, const Workspace& w, int B, int ntok) {
  AttnArgs a{};
  a.q = w.q; a.k = w.k; a.vt = w.vt; a.o = w.ao; a.ldq = m->D; a.ldk = m->kvD; a.ldo = m->D;
  a.B = B; a.N = ntok; a.Hq = m->Hq; a.Hkv = m->Hkv; a.npad = w.npad;
  a.scale_log2e = kAttnScaleLog2e; a.lens = w.lens;
  return a;
}

// The norm that consumes a block's output (norm1 of the next block, or the final norm: shift == nullptr) can ride in the
// finishing pass of a split-K fc2 (small-M buckets); likewise norm2 in that of out_proj.
struct NextNorm { const float *w, *shift, *scale; };

// Gated-residual GEMM w.x += gate * (A[M, K] W^T + bias) of out_proj (G_OUT) and fc2 (G_FC2): one launch with the EPI_RESID
// epilogue, or K slices + a finishing pass that also applies the norm `next` into w.xn where it can (*norm_done reports it)
static int resid_gemm(const jat_model* m, const Workspace& w, int site, const bf16_t* A, const bf16_t* W, int K, const float* bias,
                      const float* gate, int64_t bstride, int M, int ntok, bool folding, const NextNorm* next, bool* norm_done,
                      hipStream_t s) {
  const int D = m->D;
  *norm_done = false;
  const GemmPlan plan = plan_resid(m, site, M, K, folding, w.kpart != nullptr);
  if (plan.ksplit == 1) {
    GemmArgs e{};
    e.out = w.x; e.ldo = D; e.bias = bias; e.gate = gate; e.gate_bstride = bstride; e.ntok = ntok;
    if (folding) { e.fold_out = w.xn; e.fold_lo = w.xlo; e.fold_part = w.part; }   // feeds the norm that follows
    return jat_gemm(m, site, A, K, W, K, M, D, K, EPI_RESID, e, s, &plan);
  }
  GemmArgs p{};
  p.out = w.kpart; p.ldo = D; p.ntok = ntok; p.split_stride = (int64_t)M * D;
  JCHK(jat_gemm(m, site, A, K, W, K, M, D, K, EPI_F32, p, s, &plan));
  if (next && !folding && m->sw.fuse_finish && splitk_resid_norm_supported(D)) {   // slice sum + gate + residual + norm in one launch
    KCHK(launch_splitk_resid_norm(w.kpart, plan.ksplit, (int64_t)M * D, bias, gate, bstride, w.x, next->w, next->shift, next->scale,
                                  bstride, w.xn, M, D, ntok, m->cfg.norm_mode, s));
    *norm_done = true;
  } else {
    KCHK(launch_splitk_resid_finish(w.kpart, plan.ksplit, (int64_t)M * D, bias, gate, bstride, ntok, w.x, M, D, s));
  }
  return JAT_OK;
}

// one DiTBlock_GQA on the residual stream w.x  (jat_audiosr_v3.py:284-308); mod_l = this layer's 6D row of batch 0
// `next`: the norm that reads this block's output, *next_done reports that w.xn already holds it.
static int run_block(const jat_model* m, const Workspace& w, int l, int B, int ntok, const float* mod_l,
                     int64_t bstride, hipStream_t s, const Fold* f = nullptr, bool xn_ready = false,
                     const NextNorm* next = nullptr, bool* next_done = nullptr) {
  const int D = m->D, M = B * ntok, Nqkv = D + 2 * m->kvD;
  const LayerW& L = m->layers[l];
  if (!f && !xn_ready) KCHK(launch_norm_modulate(w.x, L.norm1, mod_l + 0 * D, mod_l + 1 * D, bstride, w.xn, M, D, ntok, m->cfg.norm_mode, s));
  const int fuse_env = m->sw.fuse_qkv_attn;   // per-handle switch (jat_model_set_switch): tests A/B the two paths on one model
  // one block per (sample, KV group): worth it only when B * Hkv blocks fill the 256 CUs (measured: +1.8 % at
  // B = 56, -5 % at B = 28); fuse_env = 2 forces it (tests).  With folded weights the sampler decided at creation.
  const bool fused_attn = f ? f->wqkv_g != nullptr
                            : (fuse_env && L.wqkv_g && !m->group_copy_stale && ntok == 128 && (B * m->Hkv >= 192 || fuse_env == 2));
  if (fused_attn) {
    // q/k/v projection + RoPE + attention of one (sample, KV group) per block: q, k, v stay in LDS
    GemmArgs a{};
    a.A = w.xn; a.lda = D; a.W = f ? f->wqkv_g + (int64_t)l * Nqkv * D : L.wqkv_g; a.ldw = D; a.M = M; a.N = m->Hkv * 448; a.K = D;
    a.out = w.ao; a.ldo = D; a.ntok = ntok; a.rope_inv_freq = m->rope_invf;
    a.attn_scale_log2e = kAttnScaleLog2e;
    if (f) { a.rs_part = w.part; a.rs_np = m->last_fold_np; a.bias = f->bq_g + (int64_t)l * Nqkv; }
    KCHK(launch_qkv_attn(a, s));
  } else {
    const GemmPlan plan = plan_qkv(m, M, D, f != nullptr, w.kpart != nullptr);
    if (plan.ksplit > 1) {
      GemmArgs p{};
      p.out = w.kpart; p.ldo = Nqkv; p.ntok = ntok; p.split_stride = (int64_t)M * Nqkv;
      JCHK(jat_gemm(m, G_QKV, w.xn, D, L.wqkv, D, M, Nqkv, D, EPI_F32, p, s, &plan));
      KCHK(launch_splitk_qkv_finish(w.kpart, plan.ksplit, (int64_t)M * Nqkv, m->rope_cos, m->rope_sin, w.q, w.k, w.vt, M, D, m->kvD,
                                    ntok, w.npad, s));
    } else {
      GemmArgs e = qkv_rope_args(m, w, ntok);
      if (f) { e.rs_part = w.part; e.bias = f->bq_i + (int64_t)l * Nqkv; }
      JCHK(jat_gemm(m, G_QKV, w.xn, D, f ? f->wqkv_i + (int64_t)l * Nqkv * D : L.wqkv, D, M, Nqkv, D, EPI_QKV_ROPE, e, s, &plan));
    }
    KCHK(launch_attention(attn_args(m, w, B, ntok), s));
  }
  const NextNorm norm2{L.norm2, mod_l + 3 * D, mod_l + 4 * D};
  bool norm2_done = false, done = false;
  JCHK(resid_gemm(m, w, G_OUT, w.ao, L.wo, D, nullptr, mod_l + 2 * D, bstride, M, ntok, f != nullptr, &norm2, &norm2_done, s));
  if (!f && !norm2_done) KCHK(launch_norm_modulate(w.x, L.norm2, mod_l + 3 * D, mod_l + 4 * D, bstride, w.xn, M, D, ntok, m->cfg.norm_mode, s));
  {
    GemmArgs e{};
    e.out = w.hm; e.ldo = m->mlp; e.bias = L.b1; e.ntok = ntok;
    if (f) { e.rs_part = w.part; e.bias = f->bf + (int64_t)l * m->mlp; }
    JCHK(jat_gemm(m, G_FC1, w.xn, D, f ? f->w1 + (int64_t)l * m->mlp * D : L.w1, D, M, m->mlp, D, EPI_BF16_GELU, e, s));
  }
  JCHK(resid_gemm(m, w, G_FC2, w.hm, L.w2, m->mlp, L.b2, mod_l + 5 * D, bstride, M, ntok, f != nullptr, next, &done, s));
  if (next_done) *next_done = done;
  return JAT_OK;
}

// First patch-embed Linear + GELU: w.h_patch = gelu(w.a_patch[rows, K] W1[:, :K]^T + b1).  pc != nullptr (CFG sampler): the
// rows are the z half shared by cond and uncond; rows r get + pc[r] inside the GELU, rows r + `rows` do not.
// In one launch, or as K slices (plan_patch) whose partials live in the MLP hidden buffer, idle until block 0's fc1.
static int patch_linear1(const jat_model* m, const Workspace& w, int rows, int K, const float* pc, int ntok, hipStream_t s) {
  const GemmPlan plan = plan_patch(m, rows, K);
  GemmArgs e{};
  e.ldo = m->bott; e.ntok = ntok;
  if (plan.ksplit > 1) {
    e.out = w.hm; e.split_stride = (int64_t)rows * m->bott;
    JCHK(jat_gemm(m, G_OTHER, w.a_patch, K, m->pe_w1, m->Kp, rows, m->bott, K, EPI_F32, e, s, &plan));
    KCHK(launch_splitk_gelu_finish((const float*)w.hm, plan.ksplit, (int64_t)rows * m->bott, m->pe_b1, pc, pc ? rows : 0, w.h_patch,
                                   m->bott, rows, m->bott, s));
    return JAT_OK;
  }
  e.out = w.h_patch; e.bias = m->pe_b1;
  if (pc) { e.dual_add = pc; e.dual_rows = rows; }
  return jat_gemm(m, G_OTHER, w.a_patch, K, m->pe_w1, m->Kp, rows, m->bott, K, EPI_BF16_GELU, e, s, &plan);
}

// The CFG sampler's fused step tail (EPI_CFG_EULER): the latent lives in patch layout (zp fp32, w.a_patch bf16) over the steps; the
// final Linear applies the CFG combine + Euler step of time t / step dt itself and writes both for the next step.
// stage != 0 (EPI_CFG_STAGE): one stage of a two-stage solver (jat_solver_plan), with the start-of-step latent z_base beside zp.
struct FusedTail {
  float* zp;
  float cfg_scale, t, dt;
  int stage = 0;              // 0: Euler step of length dt at time t; 1 / 2: first / second stage, step coefficient dt
  float* z_base = nullptr;
  float den = 0.f, a = 0.f, b = 0.f;
};

// Whole forward over B batch rows.  x_t rows are read modulo B_src and the condition is zero from batch row
// cond_zero_from on: this is how the CFG double batch [z;z],[lr;0] (infer_test_v3m2.py:154-156) is fed
// without materialising the concatenations.  mod == nullptr: compute the modulation from t [B].
static int forward_impl(const jat_model* m, const Workspace& w, const float* x_t, int B_src, const float* x_cond,
                        int cond_zero_from, const float* t, const float* mod, int64_t mod_bstride, float* x_pred,
                        int B, int T, hipStream_t s, const Fold* f = nullptr, const float* pc = nullptr,
                        const FusedTail* tail = nullptr) {
  const int ntok = (T + 3) / 4, M = B * ntok, D = m->D;
  if (!mod) {
    JCHK(time_path(m, w, t, B, s));
    // (Running this 0.55 GB weight stream on a second stream beside the patch embed was measured: 5.68 -> 5.71 ms at B = 28 —
    // its 1344 blocks and the patch GEMM's share the same CUs, nothing is gained.)
    JCHK(adaln_path(m, w.t_silu, w.mod, B, 0, m->depth, s));
    mod = w.mod;
    mod_bstride = (int64_t)m->depth * 6 * D;
  }
  // The key padding of V^T must be zero (0 * garbage could be NaN).  Nothing ever writes the padding, so the
  // sampler zeroes its private buffer once at creation (mod != nullptr path) and only the generic entry point,
  // whose workspace belongs to the caller, clears it per call.
  if (t) HIPCHK(hipMemsetAsync(w.vt, 0, w.vt_bytes, s));
  if (pc) {
    // CFG sampler: the first patch-embed Linear is linear in [z ; cond], the z part is the same for the cond and
    // uncond halves and the cond part (pc = patch(lr) @ W1[:, cond]^T, fp32) does not change over the 50 steps:
    // h_cond = gelu(S_z + pc + b1), h_uncond = gelu(S_z + b1) from ONE quarter-size GEMM (M/2 rows, K/2 deep).
    // fused tail: w.a_patch already holds patch(z), written by the previous step's final Linear (or by the run's start)
    if (!tail) KCHK(launch_patchify(x_t, nullptr, w.a_patch, B_src, B_src, B_src, m->Cin, 0, T, ntok, s, w.tvalid));
    JCHK(patch_linear1(m, w, M / 2, m->P * m->Cin, pc, ntok, s));
  } else {
    KCHK(launch_patchify(x_t, x_cond, w.a_patch, B, B_src, cond_zero_from, m->Cin, m->Cc, T, ntok, s, w.tvalid));
    JCHK(patch_linear1(m, w, M, m->Kp, nullptr, ntok, s));
  }
  {
    GemmArgs e{};
    e.out = w.x; e.ldo = D; e.bias = m->pe_b2; e.ntok = ntok;
    if (f) { e.fold_out = w.xn; e.fold_lo = w.xlo; e.fold_part = w.part; }
    JCHK(jat_gemm(m, G_OTHER, w.h_patch, m->bott, m->pe_w2, m->bott, M, D, m->bott, EPI_F32, e, s));
  }
  bool xn_ready = false;
  for (int l = 0; l < m->depth; ++l) {
    const float* mod_n = mod + (int64_t)(l + 1) * 6 * D;
    const NextNorm nn = l + 1 < m->depth ? NextNorm{m->layers[l + 1].norm1, mod_n + 0 * D, mod_n + 1 * D}
                                         : NextNorm{m->final_norm, nullptr, nullptr};
    bool done = false;
    JCHK(run_block(m, w, l, B, ntok, mod + (int64_t)l * 6 * D, mod_bstride, s, f, xn_ready, &nn, &done));
    xn_ready = done;
  }
  if (!f && !xn_ready) KCHK(launch_norm_modulate(w.x, m->final_norm, nullptr, nullptr, 0, w.xn, M, D, ntok, m->cfg.norm_mode, s));
  {
    GemmArgs e{};
    e.out = x_pred; e.bias = m->bfinal; e.ntok = ntok; e.C_out = m->Cin; e.T_orig = T;
    if (f) e.rs_part = w.part;
    if (tail) {
      e.out = tail->zp; e.ldo = m->Fout; e.ce_patch = w.a_patch; e.ce_frames = w.tvalid;
      e.ce_scale = tail->cfg_scale; e.ce_denom = 1.0f - tail->t + 1e-5f; e.ce_dt = tail->dt; e.ce_direct = !(tail->t < 0.999f);   // launch_cfg_euler
      if (tail->stage) {   // launch_cfg_stage
        e.ce_denom = tail->den; e.cs_base = tail->z_base; e.cs_a = tail->a; e.cs_b = tail->b; e.cs_save = tail->stage == 1;
      }
    }
    JCHK(jat_gemm(m, G_OTHER, w.xn, D, f ? f->wfinal : m->wfinal, D, M, m->Fout, D,
                  !tail ? EPI_UNPATCH : tail->stage ? EPI_CFG_STAGE : EPI_CFG_EULER, e, s));
  }
  return JAT_OK;
}

static int check_ready(const jat_model* m, int B, int ntok, void* ws, size_t ws_bytes, Workspace* w) {
  if (!m) return fail(JAT_E_INVALID, "null model");
  if (!m->loaded) return fail(JAT_E_STATE, "weights not loaded");
  if (B <= 0 || ntok <= 0) return fail(JAT_E_INVALID, "B and T must be positive");
  if (ntok > MAX_LEN) return fail(JAT_E_SEQLEN, "Sequence length %d exceeds max_len %d", ntok, MAX_LEN);
  *w = carve(m, B, ntok, (char*)ws);
  if (!ws || ws_bytes < w->total)
    return fail(JAT_E_STATE, "workspace too small: %zu < %zu bytes", ws_bytes, w->total);
  return JAT_OK;
}

extern "C" int jat_forward(jat_model* m, const float* x_t, const float* t, const float* x_cond, float* x_pred,
                           int32_t B, int32_t T, void* ws, size_t ws_bytes, void* stream) {
  if (T <= 0) return fail(JAT_E_INVALID, "T must be positive");
  Workspace w;
  JCHK(check_ready(m, B, (T + 3) / 4, ws, ws_bytes, &w));
  return forward_impl(m, w, x_t, B, x_cond, B, t, nullptr, 0, x_pred, B, T, (hipStream_t)stream);
}

extern "C" int jat_time_embed(jat_model* m, const float* t, float* t_emb, int32_t B, void* ws, size_t ws_bytes,
                              void* stream) {
  Workspace w;
  JCHK(check_ready(m, B, 1, ws, ws_bytes, &w));
  hipStream_t s = (hipStream_t)stream;
  JCHK(time_path(m, w, t, B, s));
  HIPCHK(hipMemcpyAsync(t_emb, w.t_emb, (size_t)B * m->D * 4, hipMemcpyDeviceToDevice, s));
  return JAT_OK;
}

extern "C" int jat_block_forward(jat_model* m, int32_t layer, const float* x, const float* t_emb, float* y, int32_t B,
                                 int32_t N, void* ws, size_t ws_bytes, void* stream) {
  Workspace w;
  JCHK(check_ready(m, B, N, ws, ws_bytes, &w));
  if (layer < 0 || layer >= m->depth) return fail(JAT_E_INVALID, "layer out of range");
  hipStream_t s = (hipStream_t)stream;
  const size_t xb = (size_t)B * N * m->D * 4;
  KCHK(launch_silu_bf16(t_emb, w.t_silu, (int64_t)B * m->D, s));
  JCHK(adaln_path(m, w.t_silu, w.mod, B, layer, 1, s));
  HIPCHK(hipMemsetAsync(w.vt, 0, w.vt_bytes, s));
  HIPCHK(hipMemcpyAsync(w.x, x, xb, hipMemcpyDeviceToDevice, s));
  JCHK(run_block(m, w, layer, B, N, w.mod, (int64_t)6 * m->D, s));
  HIPCHK(hipMemcpyAsync(y, w.x, xb, hipMemcpyDeviceToDevice, s));
  return JAT_OK;
}

extern "C" int jat_attn_forward(jat_model* m, int32_t layer, const float* x, float* y, int32_t B, int32_t N, void* ws,
                                size_t ws_bytes, void* stream) {
  Workspace w;
  JCHK(check_ready(m, B, N, ws, ws_bytes, &w));
  if (layer < 0 || layer >= m->depth) return fail(JAT_E_INVALID, "layer out of range");
  hipStream_t s = (hipStream_t)stream;
  const int D = m->D, M = B * N;
  const LayerW& L = m->layers[layer];
  HIPCHK(hipMemsetAsync(w.vt, 0, w.vt_bytes, s));
  KCHK(launch_norm_modulate(x, nullptr, nullptr, nullptr, 0, w.xn, M, D, N, 2, s));  // plain bf16 cast
  JCHK(jat_gemm(m, G_QKV, w.xn, D, L.wqkv, D, M, D + 2 * m->kvD, D, EPI_QKV_ROPE, qkv_rope_args(m, w, N), s));
  KCHK(launch_attention(attn_args(m, w, B, N), s));
  {
    GemmArgs e{};
    e.out = y; e.ldo = D; e.ntok = N;
    JCHK(jat_gemm(m, G_OUT, w.ao, D, L.wo, D, M, D, D, EPI_F32, e, s));
  }
  return JAT_OK;
}

// ---------------------------------------------------------------------------------------------------------
// sampler
// ---------------------------------------------------------------------------------------------------------
struct jat_sampler {
  jat_model* m;
  int B, T, Bf;  // Bf = batch rows per forward (2B with CFG)
  float cfg_scale;
  bool use_cfg;
  std::vector<jat_solver_eval> plan;   // the model evaluations of a run, in order (jat_solver_plan)
  std::vector<float> times;            // the distinct evaluation times: rows of mod_table, entries of the folded-weight table
  float* z_base = nullptr;             // two-stage solvers: the latent at the start of the step, in the layout z / zp has
  char* blob = nullptr;   // private device allocation
  float *z, *lr, *xpred, *mod_table, *ts_dev;
  float* zp = nullptr;               // fused tail: the latent in patch layout [B ntok, 4 C] over the steps of a run
  bool tail_fused = false;           // the final Linear applies CFG + Euler (EPI_CFG_EULER); no cfg_euler / per-step patchify launches
  std::shared_ptr<FoldTable> fold;   // per-step folded weights (RMSNorm models), shared through the model's cache
  bool fused_attn = false;           // this bucket runs the fused QKV+attention kernel (group-major folded weights)
  float* pc = nullptr;   // CFG: patch(lr) @ W1[:, cond]^T, recomputed once per run (split patch embed)
  int* lens_dev = nullptr;   // [Bf] valid tokens per batch row (default: ntok), read by the attention kernel of the graph
  int* frames_dev = nullptr; // [B] valid frames per row (default: T), read by the patchify kernels
  bool folded = false;
  void* ws;
  size_t ws_bytes;
  Workspace w;
  hipStream_t cap_stream = nullptr;
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
};

// torch.linspace(0, 1, n) in fp32 as PyTorch evaluates it (step = fp32(1/(n-1)); first half start+step*i,
// second half end-step*(n-1-i), one rounding each) — pinned by tests/golden/misc.npz `linspace51`.
static void linspace01(int n, std::vector<float>& out) {
  out.resize(n);
  const float step = 1.0f / (float)(n - 1);
  for (int i = 0; i < n; ++i)
    out[i] = i < n / 2 ? (float)((double)step * i) : (float)(1.0 - (double)step * (n - 1 - i));
}

// The evaluation list of a solver over a time grid (include/jat_hip.h).  Pure host code.
//   euler:    z' = z + dt v(z, t)                                                       (the reference's step, direct from t >= 0.999)
//   midpoint: z~ = z + h v(z, t);   z' = z_base + dt v(z~, t + h)                       h = dt / 2
//   heun:     z~ = z + dt v(z, t);  z' = z_base / 2 + z~ / 2 + h v(z~, t_next)
// A step whose second time is not < 0.999 is taken as the Euler step: v = (x - z) / (1 - t + 1e-5) is singular at t = 1.
static uint32_t f32_bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }
extern "C" int jat_solver_plan(const float* times, int32_t n, int32_t solver, jat_solver_eval* evals, int32_t cap, int32_t* n_evals,
                               float* distinct, int32_t* n_distinct) {
  if (n < 2) return fail(JAT_E_INVALID, "a time grid needs at least two values, got %d", n);
  if (solver != JAT_SOLVER_EULER && solver != JAT_SOLVER_MIDPOINT && solver != JAT_SOLVER_HEUN)
    return fail(JAT_E_INVALID, "unknown solver %d", solver);
  std::vector<float> lin;
  if (!times) { linspace01(n, lin); times = lin.data(); }
  if (!(times[0] == 0.0f) || !(times[n - 1] == 1.0f)) return fail(JAT_E_INVALID, "the time grid must start at 0 and end at 1");
  for (int i = 0; i + 1 < n; ++i)
    if (!(times[i + 1] > times[i])) return fail(JAT_E_INVALID, "the time grid must be strictly increasing (index %d)", i + 1);
  std::vector<jat_solver_eval> ev;
  std::vector<float> dis;
  std::map<uint32_t, int> index;
  auto push = [&](float t, int stage, float a, float b, float c) {
    auto it = index.find(f32_bits(t));
    if (it == index.end()) { it = index.emplace(f32_bits(t), (int)dis.size()).first; dis.push_back(t); }
    jat_solver_eval e{};
    e.t = t; e.time_index = it->second; e.den = 1.0f - t + 1e-5f; e.a = a; e.b = b; e.c = c;
    e.stage = stage; e.save = stage == 1; e.direct = stage == 0 && !(t < 0.999f);
    ev.push_back(e);
  };
  for (int i = 0; i + 1 < n; ++i) {
    const float t = times[i], dt = times[i + 1] - t, h = 0.5f * dt;
    const float t2 = solver == JAT_SOLVER_MIDPOINT ? t + h : times[i + 1];
    if (solver == JAT_SOLVER_EULER || !(t2 < 0.999f)) { push(t, 0, 0.0f, 1.0f, dt); continue; }
    if (solver == JAT_SOLVER_MIDPOINT) { push(t, 1, 0.0f, 1.0f, h); push(t2, 2, 1.0f, 0.0f, dt); }
    else { push(t, 1, 0.0f, 1.0f, dt); push(t2, 2, 0.5f, 0.5f, h); }
  }
  if (n_evals) *n_evals = (int32_t)ev.size();
  if (n_distinct) *n_distinct = (int32_t)dis.size();
  if ((evals && cap < (int32_t)ev.size()) || (distinct && cap < (int32_t)dis.size()))
    return fail(JAT_E_INVALID, "room for %d entries, the plan has %zu evaluations", cap, ev.size());
  if (evals) std::copy(ev.begin(), ev.end(), evals);
  if (distinct) std::copy(dis.begin(), dis.end(), distinct);
  return JAT_OK;
}

// pc = patch(lr) @ W1[:, cond columns]^T (fp32, no bias): once per run, before the captured steps
static int sampler_cond_part(jat_sampler* sp, hipStream_t s) {
  if (!sp->pc) return JAT_OK;
  jat_model* m = sp->m;
  const int ntok = (sp->T + 3) / 4, Kc = m->P * m->Cc;
  KCHK(launch_patchify(sp->lr, nullptr, sp->w.a_patch, sp->B, sp->B, sp->B, m->Cc, 0, sp->T, ntok, s, sp->w.tvalid));
  GemmArgs e{};
  e.out = sp->pc; e.ldo = m->bott; e.ntok = ntok;
  return jat_gemm(m, G_OTHER, sp->w.a_patch, Kc, m->pe_w1 + (int64_t)m->P * m->Cin, m->Kp, sp->B * ntok, m->bott, Kc, EPI_F32, e, s);
}

// Around the steps of a run (outside the captured graph).  begin: the condition part, then (fused tail) the latent into patch
// layout, fp32 for the update and bf16 as the first step's patch operand (sampler_cond_part uses a_patch as scratch: after it);
// end: back to [B, C, T].
static int sampler_begin(jat_sampler* sp, hipStream_t s) {
  JCHK(sampler_cond_part(sp, s));
  if (!sp->tail_fused) return JAT_OK;
  const jat_model* m = sp->m;
  KCHK(launch_patch_f32(sp->z, sp->zp, sp->B, m->Cin, sp->T, s));
  KCHK(launch_patchify(sp->z, nullptr, sp->w.a_patch, sp->B, sp->B, sp->B, m->Cin, 0, sp->T, sp->T / 4, s, sp->w.tvalid));
  return JAT_OK;
}
static int sampler_end(jat_sampler* sp, hipStream_t s) {
  if (sp->tail_fused) KCHK(launch_unpatch_f32(sp->zp, sp->z, sp->B, sp->m->Cin, sp->T, s));
  return JAT_OK;
}

// The evaluations of the plan in order.  warm_up: only the first evaluation of each launch kind (Euler step / solver stage): the
// eager pass before the capture that sets the kernels' function attributes.
static int sampler_steps(jat_sampler* sp, hipStream_t s, bool warm_up = false) {
  jat_model* m = sp->m;
  const int64_t n_half = (int64_t)sp->B * m->Cin * sp->T;
  const int64_t row = (int64_t)m->depth * 6 * m->D;
  bool seen[2] = {false, false};
  for (const jat_solver_eval& ev : sp->plan) {
    if (warm_up) {
      if (seen[ev.stage != 0]) continue;
      seen[ev.stage != 0] = true;
    }
    const int i = ev.time_index;
    const float t_curr = ev.t, dt = ev.c;
    Fold f{};
    if (sp->folded) {
      const FoldTable& ft = *sp->fold;
      const int64_t Nqkv = m->D + 2 * m->kvD, dl = m->depth;
      if (sp->fused_attn) { f.wqkv_g = ft.qkv_g + (int64_t)i * dl * Nqkv * m->D; f.bq_g = ft.bq_g + (int64_t)i * dl * Nqkv; }
      else { f.wqkv_i = ft.qkv_i + (int64_t)i * dl * Nqkv * m->D; f.bq_i = ft.bq_i + (int64_t)i * dl * Nqkv; }
      f.w1 = ft.w1 + (int64_t)i * dl * m->mlp * m->D;
      f.bf = ft.bf + (int64_t)i * dl * m->mlp;
      f.wfinal = ft.wfinal;
    }
    const FusedTail tail{sp->zp, sp->cfg_scale, t_curr, dt, ev.stage, sp->z_base, ev.den, ev.a, ev.b};
    JCHK(forward_impl(m, sp->w, sp->z, sp->B, sp->lr, sp->B, nullptr, sp->mod_table + i * row, 0, sp->xpred, sp->Bf,
                      sp->T, s, sp->folded ? &f : nullptr, sp->pc, sp->tail_fused ? &tail : nullptr));
    if (!sp->tail_fused && !ev.stage) KCHK(launch_cfg_euler(sp->xpred, sp->z, sp->cfg_scale, t_curr, dt, sp->use_cfg ? 1 : 0, n_half, s));
    if (!sp->tail_fused && ev.stage)
      KCHK(launch_cfg_stage(sp->xpred, sp->z, sp->z_base, sp->cfg_scale, ev.den, ev.a, ev.b, ev.c, sp->use_cfg ? 1 : 0, ev.save, n_half, s));
  }
  return JAT_OK;
}

// Build (or extend with the missing QKV layout) the folded-weight table of `steps` steps from the modulation table
// mod [steps][depth*6D] (fp32, device).  Everything is enqueued on s; the caller synchronises.  On an allocation
// failure the sampler simply runs un-folded (norm kernels).
static int fold_alloc(FoldTable& ft, void** p, size_t bytes) {
  if (hipMalloc(p, bytes) != hipSuccess) { (void)hipGetLastError(); return fail(JAT_E_HIP, "hipMalloc(%zu) for the folded weights", bytes); }
  ft.allocs.push_back(*p);
  return JAT_OK;
}
static int build_fold_table_impl(jat_model* m, FoldTable& ft, int steps, const float* mod, bool group_major, bf16_t* sh_bf16,
                                 hipStream_t s, bool need_w1, bool need_qkv);
static int build_fold_table(jat_model* m, FoldTable& ft, int steps, const float* mod, bool group_major, bf16_t* sh_bf16,
                            hipStream_t s) {
  const bool need_w1 = ft.w1 == nullptr;
  const bool need_qkv = group_major ? ft.qkv_g == nullptr : ft.qkv_i == nullptr;
  const size_t keep = ft.allocs.size();
  const int rc = build_fold_table_impl(m, ft, steps, mod, group_major, sh_bf16, s, need_w1, need_qkv);
  if (rc != JAT_OK) {
    // undo THIS call's allocations and pointers: what earlier calls built (and other samplers hold) stays valid, and no
    // half-built part is left looking finished
    (void)hipStreamSynchronize(s);
    while (ft.allocs.size() > keep) { (void)hipFree(ft.allocs.back()); ft.allocs.pop_back(); }
    if (need_w1) { ft.w1 = nullptr; ft.bf = nullptr; ft.wfinal = nullptr; }
    if (need_qkv) { if (group_major) { ft.qkv_g = nullptr; ft.bq_g = nullptr; } else { ft.qkv_i = nullptr; ft.bq_i = nullptr; } }
  }
  return rc;
}
static int build_fold_table_impl(jat_model* m, FoldTable& ft, int steps, const float* mod, bool group_major, bf16_t* sh_bf16,
                                 hipStream_t s, bool need_w1, bool need_qkv) {
  const int D = m->D, kvD = m->kvD, mlp = m->mlp, depth = m->depth, Nqkv = D + 2 * kvD;
  const int64_t mrow = (int64_t)depth * 6 * D;
  if (need_w1) {
    JCHK(fold_alloc(ft, (void**)&ft.w1, (size_t)steps * depth * mlp * D * 2));
    JCHK(fold_alloc(ft, (void**)&ft.bf, (size_t)steps * depth * mlp * 4));
    JCHK(fold_alloc(ft, (void**)&ft.wfinal, (size_t)m->Fout * D * 2));
    KCHK(launch_fold_weight(m->wfinal32, m->final_norm, nullptr, ft.wfinal, m->Fout, D, 0, s));
  }
  bf16_t* qkv = nullptr;
  float* bq = nullptr;
  if (need_qkv) {
    JCHK(fold_alloc(ft, (void**)&qkv, (size_t)steps * depth * Nqkv * D * 2));
    JCHK(fold_alloc(ft, (void**)&bq, (size_t)steps * depth * Nqkv * 4));
    if (group_major) { ft.qkv_g = qkv; ft.bq_g = bq; } else { ft.qkv_i = qkv; ft.bq_i = bq; }
  }
  ft.steps = steps;
  for (int l = 0; l < depth; ++l) {
    const LayerW& L = m->layers[l];
    for (int i = 0; i < steps; ++i) {
      const float* mod_il = mod + i * mrow + (int64_t)l * 6 * D;   // shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp
      if (need_qkv) {
        bf16_t* dst = qkv + ((int64_t)i * depth + l) * Nqkv * D;
        if (group_major) {   // per KV head g: its 5 q heads, its k head, its v head (the layout of L.wqkv_g)
          for (int g = 0; g < m->Hkv; ++g) {
            bf16_t* dg = dst + (int64_t)g * 448 * D;
            KCHK(launch_fold_weight(L.q32 + (int64_t)g * 320 * D, L.norm1, mod_il + D, dg, 320, D, 1, s));
            KCHK(launch_fold_weight(L.k32 + (int64_t)g * 64 * D, L.norm1, mod_il + D, dg + (int64_t)320 * D, 64, D, 1, s));
            KCHK(launch_fold_weight(L.v32 + (int64_t)g * 64 * D, L.norm1, mod_il + D, dg + (int64_t)384 * D, 64, D, 0, s));
          }
        } else {
          KCHK(launch_fold_weight(L.q32, L.norm1, mod_il + D, dst, D, D, 1, s));
          KCHK(launch_fold_weight(L.k32, L.norm1, mod_il + D, dst + (int64_t)D * D, kvD, D, 1, s));
          KCHK(launch_fold_weight(L.v32, L.norm1, mod_il + D, dst + (int64_t)(D + kvD) * D, kvD, D, 0, s));
        }
      }
      if (need_w1) KCHK(launch_fold_weight(L.w132, L.norm2, mod_il + 4 * D, ft.w1 + ((int64_t)i * depth + l) * mlp * D, mlp, D, 0, s));
    }
    // shift @ W^T for all steps of this layer in one skinny GEMM each (un-folded packed weights, fp32 accumulate)
    if (need_qkv) {
      KCHK(launch_gather_cast_rows(mod + (int64_t)l * 6 * D, mrow, sh_bf16, steps, D, s));
      GemmArgs e{};
      e.out = bq + (int64_t)l * Nqkv; e.ldo = (int64_t)depth * Nqkv; e.ntok = 1;
      JCHK(jat_gemm(m, G_OTHER, sh_bf16, D, group_major ? L.wqkv_g : L.wqkv, D, steps, Nqkv, D, EPI_F32, e, s));
    }
    if (need_w1) {
      KCHK(launch_gather_cast_rows(mod + (int64_t)l * 6 * D + 3 * D, mrow, sh_bf16, steps, D, s));
      GemmArgs e{};
      e.out = ft.bf + (int64_t)l * mlp; e.ldo = (int64_t)depth * mlp; e.bias = L.b1; e.ntok = 1;
      JCHK(jat_gemm(m, G_OTHER, sh_bf16, D, L.w1, D, steps, mlp, D, EPI_F32, e, s));
    }
  }
  return JAT_OK;
}

extern "C" void jat_sampler_destroy(jat_sampler* sp) {
  if (!sp) return;
  if (sp->exec) (void)hipGraphExecDestroy(sp->exec);
  if (sp->graph) (void)hipGraphDestroy(sp->graph);
  if (sp->cap_stream) (void)hipStreamDestroy(sp->cap_stream);
  if (sp->blob) (void)hipFree(sp->blob);
  delete sp;
}

extern "C" int jat_sampler_create(jat_model* m, int32_t B, int32_t T, int32_t steps, float cfg_scale,
                                  jat_sampler** out) {
  if (steps <= 0) return fail(JAT_E_INVALID, "B, T, steps must be positive");
  return jat_sampler_create_ex(m, B, T, nullptr, steps + 1, JAT_SOLVER_EULER, cfg_scale, out);
}

extern "C" int jat_sampler_create_ex(jat_model* m, int32_t B, int32_t T, const float* times, int32_t n_times, int32_t solver,
                                     float cfg_scale, jat_sampler** out) {
  if (!m || !out) return fail(JAT_E_INVALID, "null argument");
  if (!m->loaded) return fail(JAT_E_STATE, "weights not loaded");
  if (B <= 0 || T <= 0) return fail(JAT_E_INVALID, "B, T, steps must be positive");
  // the LR latent is the condition of every step and has the shape of the sampled latent (infer_test_v3m2.py:107-185)
  if (m->Cc != m->Cin)
    return fail(JAT_E_INVALID, "the sampler conditions on a latent of the sampled shape: cond_channels (%d) must equal input_channels (%d)",
                m->Cc, m->Cin);
  // the evaluation list first: it validates the grid and the solver, and sizes the tables (one row / entry per distinct time)
  std::vector<jat_solver_eval> plan((size_t)(n_times > 1 ? 2 * (n_times - 1) : 0));
  std::vector<float> distinct(plan.size());
  int32_t n_evals = 0, n_distinct = 0;
  JCHK(jat_solver_plan(times, n_times, solver, plan.data(), (int32_t)plan.size(), &n_evals, distinct.data(), &n_distinct));
  plan.resize((size_t)n_evals);
  distinct.resize((size_t)n_distinct);
  const int steps = n_distinct;   // rows of the modulation table and entries of the folded-weight table
  const int ntok = (T + 3) / 4;
  if (ntok > MAX_LEN) return fail(JAT_E_SEQLEN, "Sequence length %d exceeds max_len %d", ntok, MAX_LEN);
  // The tables and the captured graph are built on a private stream: order them after everything already enqueued on
  // the caller's streams (e.g. an asynchronous weight re-pack).  Creation is a slow path; a device sync is the simple order.
  HIPCHK(hipDeviceSynchronize());
  jat_sampler* sp = new jat_sampler();
  sp->m = m; sp->B = B; sp->T = T; sp->cfg_scale = cfg_scale;
  sp->plan = plan; sp->times = distinct;
  sp->use_cfg = cfg_scale != 1.0f;  // infer_test_v3m2.py:139
  sp->Bf = sp->use_cfg ? 2 * B : B;
  const bool two_stage = std::any_of(plan.begin(), plan.end(), [](const jat_solver_eval& e) { return e.stage != 0; });

  const size_t lat = (size_t)B * m->Cin * T * 4;
  const size_t row = (size_t)m->depth * 6 * m->D;
  const int Bws = sp->Bf > steps ? sp->Bf : steps;  // the table precompute runs the time path on `steps` rows
  const size_t ws_bytes = carve(m, Bws, ntok, nullptr).total;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off += align_up(bytes, 256); return o; };
  // Fused step tail ("fuse_euler"): CFG with the split patch embed (a_patch is then exactly patch(z), [B ntok, 4 C]), whole patches,
  // and a final-Linear tile that has the epilogue (its A rows are addressed by 32-bit byte offsets); anything else keeps the
  // unpatchify store + cfg_euler + patchify launches.  The tile must have it whether or not the folded-weight table gets built below.
  const int Mf = sp->Bf * ntok;
  sp->tail_fused = m->sw.fuse_euler && sp->use_cfg && m->sw.split_patch && T % 4 == 0 && (int64_t)Mf * m->D * 2 < (1ll << 31) &&
                   gemm_cfg_euler_supported(plan_gemm(m, G_OTHER, Mf, m->Fout, 1, true).variant) &&
                   gemm_cfg_euler_supported(plan_gemm(m, G_OTHER, Mf, m->Fout, 1, false).variant);
  // the fused tail keeps the latent in patch layout (zp) and never stores x_pred; the separate launches need x_pred and no zp
  const size_t o_z = take(lat), o_lr = take(lat), o_xp = take(sp->tail_fused ? 0 : (size_t)sp->Bf * m->Cin * T * 4);
  const size_t o_tab = take((size_t)steps * row * 4), o_ts = take((size_t)steps * 4), o_ws = take(ws_bytes);
  // Norm folding (default on for RMSNorm models; JAT_FOLD_NORM=0 keeps the norm kernels): decided per sampler.
  sp->folded = plan_fold_norms(m, sp->Bf * ntok);
  const int fuse_env = m->sw.fuse_qkv_attn;
  sp->fused_attn = fuse_env && m->Hq / m->Hkv == 5 && !m->group_copy_stale && ntok == 128 && (sp->Bf * m->Hkv >= 192 || fuse_env == 2);
  const size_t o_sh = take((size_t)steps * m->D * 2);
  const size_t o_lens = take((size_t)sp->Bf * 4), o_frames = take((size_t)B * 4);
  const size_t o_pc = take((size_t)B * ntok * m->bott * 4);
  const size_t o_zp = take(sp->tail_fused ? lat : 0);
  const size_t o_zb = take(two_stage ? lat : 0);
  hipError_t e = hipMalloc((void**)&sp->blob, off);
  if (e != hipSuccess) { delete sp; return fail(JAT_E_HIP, "hipMalloc(%zu): %s", off, hipGetErrorString(e)); }
  sp->z = (float*)(sp->blob + o_z); sp->lr = (float*)(sp->blob + o_lr);
  sp->xpred = sp->tail_fused ? nullptr : (float*)(sp->blob + o_xp);
  sp->mod_table = (float*)(sp->blob + o_tab); sp->ts_dev = (float*)(sp->blob + o_ts);
  sp->ws = sp->blob + o_ws; sp->ws_bytes = ws_bytes;
  bf16_t* sh_bf16 = (bf16_t*)(sp->blob + o_sh);
  sp->lens_dev = (int*)(sp->blob + o_lens);
  sp->frames_dev = (int*)(sp->blob + o_frames);
  if (sp->use_cfg && m->sw.split_patch) sp->pc = (float*)(sp->blob + o_pc);
  if (sp->tail_fused) sp->zp = (float*)(sp->blob + o_zp);
  if (two_stage) sp->z_base = (float*)(sp->blob + o_zb);

  int rc = JAT_OK;
  auto bail = [&](int code) { jat_sampler_destroy(sp); return code; };
  if (hipStreamCreateWithFlags(&sp->cap_stream, hipStreamNonBlocking) != hipSuccess)
    return bail(fail(JAT_E_HIP, "hipStreamCreate failed"));
  hipStream_t s = sp->cap_stream;

  // modulation table [distinct times, depth*6D]: every row of an evaluation shares its t (infer_test_v3m2.py:150)
  {
    Workspace wt = carve(m, steps, ntok, (char*)sp->ws);
    if (hipMemcpyAsync(sp->ts_dev, sp->times.data(), (size_t)steps * 4, hipMemcpyHostToDevice, s) != hipSuccess)
      return bail(fail(JAT_E_HIP, "memcpy ts"));
    if ((rc = time_path(m, wt, sp->ts_dev, steps, s)) != JAT_OK) return bail(rc);
    if ((rc = adaln_path(m, wt.t_silu, sp->mod_table, steps, 0, m->depth, s)) != JAT_OK) return bail(rc);
    if (sp->folded) {
      // folded weights per distinct time: shared by every sampler of this model with the same list of times (model-level cache:
      // Heun over a grid shares Euler's).  The cache keeps at most TWO lists alive on its own (a table is ~0.5 GB per step for v3mod2: 25 GB at 50 steps,
      // 50 GB at the 100 steps the reference README also offers); tables that a live sampler still holds stay until it is destroyed.
      std::vector<uint32_t> key(sp->times.size());
      for (size_t i = 0; i < key.size(); ++i) key[i] = f32_bits(sp->times[i]);
      for (auto it = m->fold_cache.begin(); it != m->fold_cache.end() && m->fold_cache.size() >= 2;)
        it = (it->first != key && it->second.use_count() == 1) ? m->fold_cache.erase(it) : std::next(it);
      const size_t Nq = (size_t)m->D + 2 * m->kvD;
      const size_t need = (size_t)steps * m->depth * ((Nq + m->mlp) * m->D * 2 + (Nq + m->mlp) * 4) + (size_t)m->Fout * m->D * 2;
      const bool over_cap = m->sw.fold_cap_mb > 0 && need > (size_t)m->sw.fold_cap_mb * 1048576;   // "fold_cap_mb": operator's bound
      std::shared_ptr<FoldTable>& slot = m->fold_cache[key];
      if (!slot) slot = std::make_shared<FoldTable>();
      if (over_cap || build_fold_table(m, *slot, steps, sp->mod_table, sp->fused_attn, sh_bf16, s) != JAT_OK) {
        (void)hipStreamSynchronize(s);
        // over the cap or out of memory: run this sampler with the norm kernels.  What was already built stays for the samplers
        // that hold it; an EMPTY entry is dropped so that a later, smaller request starts clean
        if (!slot->w1 && !slot->qkv_g && !slot->qkv_i) m->fold_cache.erase(key);
        sp->folded = false;
      } else {
        sp->fold = slot;
      }
    }
    if (hipStreamSynchronize(s) != hipSuccess) return bail(fail(JAT_E_HIP, "sync after table build"));
  }
  sp->w = carve(m, sp->Bf, ntok, (char*)sp->ws);
  if (hipMemsetAsync(sp->w.vt, 0, sp->w.vt_bytes, s) != hipSuccess) return bail(fail(JAT_E_HIP, "memset vt"));
  {  // every row attends to all of its ntok keys until jat_sampler_set_lengths says otherwise; the fused QKV+attention
     // kernel (ntok == 128) has no key mask and is never combined with lengths
    std::vector<int> full((size_t)sp->Bf, ntok), fullT((size_t)B, T);
    if (hipMemcpyAsync(sp->lens_dev, full.data(), full.size() * 4, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(sp->frames_dev, fullT.data(), fullT.size() * 4, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
      return bail(fail(JAT_E_HIP, "lengths upload"));
    if (!sp->fused_attn) { sp->w.lens = sp->lens_dev; sp->w.tvalid = sp->frames_dev; }
  }

  // one eager pass first: sets every kernel's function attributes outside of capture and validates launches
  if (hipMemsetAsync(sp->z, 0, lat, s) != hipSuccess || hipMemsetAsync(sp->lr, 0, lat, s) != hipSuccess)
    return bail(fail(JAT_E_HIP, "memset"));
  if (two_stage && hipMemsetAsync(sp->z_base, 0, lat, s) != hipSuccess) return bail(fail(JAT_E_HIP, "memset"));
  {
    if ((rc = sampler_begin(sp, s)) != JAT_OK) return bail(rc);
    rc = sampler_steps(sp, s, true);
    if (rc == JAT_OK) rc = sampler_end(sp, s);
    if (rc != JAT_OK) return bail(rc);
    if (hipStreamSynchronize(s) != hipSuccess)
      return bail(fail(JAT_E_HIP, "eager warm-up step failed: %s", hipGetErrorString(hipGetLastError())));
  }
  // capture all the plan's forwards + updates into one graph
  if (hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed) != hipSuccess)
    return bail(fail(JAT_E_HIP, "hipStreamBeginCapture failed"));
  rc = sampler_steps(sp, s);
  e = hipStreamEndCapture(s, &sp->graph);
  if (rc != JAT_OK) return bail(rc);
  if (e != hipSuccess) return bail(fail(JAT_E_HIP, "hipStreamEndCapture: %s", hipGetErrorString(e)));
  e = hipGraphInstantiate(&sp->exec, sp->graph, nullptr, nullptr, 0);
  if (e != hipSuccess) return bail(fail(JAT_E_HIP, "hipGraphInstantiate: %s", hipGetErrorString(e)));
  *out = sp;
  return JAT_OK;
}

// what this sampler's captured graph runs: folded != 0 = per-step folded weights (no norm kernels), fused_attn != 0 = the fused
// QKV + RoPE + attention kernel, fold_bytes = size of the folded-weight table it shares through the model (0 when not folded)
extern "C" int jat_sampler_info(const jat_sampler* sp, int32_t* folded, int32_t* fused_attn, int64_t* fold_bytes) {
  if (!sp) return fail(JAT_E_INVALID, "null sampler");
  if (folded) *folded = sp->folded ? 1 : 0;
  if (fused_attn) *fused_attn = sp->fused_attn ? 1 : 0;
  if (fold_bytes) {
    const jat_model* m = sp->m;
    const size_t Nq = (size_t)m->D + 2 * m->kvD;
    *fold_bytes = sp->folded ? (int64_t)((size_t)sp->times.size() * m->depth * ((Nq + m->mlp) * m->D * 2 + (Nq + m->mlp) * 4) + (size_t)m->Fout * m->D * 2) : 0;
  }
  return JAT_OK;
}

extern "C" int jat_sampler_tail_fused(const jat_sampler* sp) { return sp && sp->tail_fused ? 1 : 0; }

extern "C" int jat_sampler_set_lengths(jat_sampler* sp, const int32_t* frames, int32_t n, void* stream) {
  if (!sp || !frames) return fail(JAT_E_INVALID, "null argument");
  if (n != sp->B) return fail(JAT_E_INVALID, "need one length per batch row (%d), got %d", sp->B, n);
  std::vector<int> tok((size_t)sp->Bf);
  bool all_full = true;
  for (int b = 0; b < sp->B; ++b) {
    if (frames[b] <= 0 || frames[b] > sp->T) return fail(JAT_E_INVALID, "length %d of row %d outside (0, %d]", frames[b], b, sp->T);
    tok[b] = (frames[b] + 3) / 4;                       // the reference pads a chunk to a multiple of 4 frames (:435-439)
    if (sp->use_cfg) tok[sp->B + b] = tok[b];           // CFG double batch [cond ; uncond]
    all_full = all_full && frames[b] == sp->T;          // per FRAME: the fused buckets wire no frame mask into patchify either
  }
  if (sp->fused_attn && !all_full)
    return fail(JAT_E_STATE, "this bucket runs the fused QKV+attention kernel (128 tokens), which has no key mask");
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipMemcpyAsync(sp->lens_dev, tok.data(), tok.size() * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(sp->frames_dev, frames, (size_t)sp->B * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));                      // `tok` / `frames` are host memory of the caller
  return JAT_OK;
}

extern "C" int jat_sampler_run(jat_sampler* sp, const float* lr_latent, const float* z0, float* z_out,
                               int32_t use_graph, void* stream) {
  if (!sp || !lr_latent || !z0 || !z_out) return fail(JAT_E_INVALID, "null argument");
  hipStream_t s = (hipStream_t)stream;
  const size_t lat = (size_t)sp->B * sp->m->Cin * sp->T * 4;
  HIPCHK(hipMemcpyAsync(sp->lr, lr_latent, lat, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipMemcpyAsync(sp->z, z0, lat, hipMemcpyDeviceToDevice, s));
  JCHK(sampler_begin(sp, s));
  if (use_graph) {
    HIPCHK(hipGraphLaunch(sp->exec, s));
  } else {
    JCHK(sampler_steps(sp, s));
  }
  JCHK(sampler_end(sp, s));
  HIPCHK(hipMemcpyAsync(z_out, sp->z, lat, hipMemcpyDeviceToDevice, s));
  return JAT_OK;
}

extern "C" int jat_cfg_euler_step(const float* x_pred_2B, float* z, float cfg_scale, float t, float dt, int32_t B,
                                  int32_t C, int32_t T, void* stream) {
  KCHK(launch_cfg_euler(x_pred_2B, z, cfg_scale, t, dt, cfg_scale != 1.0f ? 1 : 0, (int64_t)B * C * T,
                        (hipStream_t)stream));
  return JAT_OK;
}

extern "C" int jat_cfg_stage_step(const float* x_pred_2B, float* z, float* z_base, float cfg_scale, float t, float a, float b,
                                  float c, int32_t save, int32_t B, int32_t C, int32_t T, void* stream) {
  if (!x_pred_2B || !z || !z_base || B <= 0 || C <= 0 || T <= 0) return fail(JAT_E_INVALID, "bad argument");
  KCHK(launch_cfg_stage(x_pred_2B, z, z_base, cfg_scale, 1.0f - t + 1e-5f, a, b, c, cfg_scale != 1.0f ? 1 : 0, save ? 1 : 0,
                        (int64_t)B * C * T, (hipStream_t)stream));
  return JAT_OK;
}

extern "C" int jat_channel_affine(const float* in, const float* mean, const float* std, float* out, int32_t B, int32_t C,
                                  int32_t T, int32_t inverse, void* stream) {
  KCHK(launch_channel_affine(in, mean, std, out, B, C, T, inverse, (hipStream_t)stream));
  return JAT_OK;
}
extern "C" int jat_crossfade_pair(const float* prev, int32_t Tp, const float* cur, int32_t Tc, int32_t overlap,
                                  float* out, int32_t rows, void* stream) {
  KCHK(launch_crossfade_pair(prev, Tp, cur, Tc, overlap, out, rows, (hipStream_t)stream));
  return JAT_OK;
}

// ---------------------------------------------------------------------------------------------------------
// per-kernel entry points
// ---------------------------------------------------------------------------------------------------------
extern "C" int jat_k_norm_modulate(const float* x, const float* w, const float* shift, const float* scale,
                                   int64_t mod_bstride, uint16_t* y, int32_t M, int32_t D, int32_t rows_per_batch,
                                   int32_t norm_mode, void* stream) {
  KCHK(launch_norm_modulate(x, w, shift, scale, mod_bstride, y, M, D, rows_per_batch, norm_mode, (hipStream_t)stream));
  return JAT_OK;
}
// -DJAT_TIMELINE build (tools/tl_probe.py): JAT_GEMM_TIMELINE = device address the GEMM kernels write their stamps to
static unsigned long long* timeline_out() {
  const char* d = getenv("JAT_GEMM_TIMELINE");
  return d ? (unsigned long long*)strtoull(d, nullptr, 0) : nullptr;
}
extern "C" int jat_k_gemm(const uint16_t* A, const uint16_t* W, const float* bias, void* C, int32_t M, int32_t N,
                          int32_t K, int32_t epilogue, const float* gate, int64_t gate_bstride, int32_t rows_per_batch,
                          int32_t variant, void* stream) {
  if (epilogue < 0 || epilogue > EPI_RESID) return fail(JAT_E_INVALID, "epilogue must be 0..3");
  GemmArgs a{};
  a.A = A; a.W = W; a.lda = K; a.ldw = K; a.M = M; a.N = N; a.K = K;
  a.out = C; a.ldo = N; a.bias = bias; a.gate = gate; a.gate_bstride = gate_bstride;
  a.ntok = rows_per_batch > 0 ? rows_per_batch : 1;
  a.dbg_out = timeline_out();
  KCHK(launch_gemm(a, epilogue, variant, (hipStream_t)stream));
  return JAT_OK;
}
// split-K slices of C = A W^T: parts[z][M][N] fp32 = the sum over K columns [z K/ksplit, (z+1) K/ksplit); the caller (or the
// finishing passes of elementwise.hip) adds the slices in order.  The un-folded forward's fc2 / out_proj use it when their
// tiles leave CUs idle (plan_resid); variant 39 = the 224 x 160 k-step-pair tile (M % 224 == 0, N % 160 == 0).
extern "C" int jat_k_gemm_splitk(const uint16_t* A, const uint16_t* W, float* parts, int32_t M, int32_t N, int32_t K,
                                 int32_t ksplit, int32_t variant, void* stream) {
  if (!A || !W || !parts || M <= 0 || N <= 0 || ksplit < 2 || K % (64 * ksplit) != 0) return fail(JAT_E_INVALID, "bad argument");
  if (!gemm_variant(variant)) return fail(JAT_E_INVALID, "unknown variant");
  GemmArgs a{};
  a.A = A; a.W = W; a.lda = K; a.ldw = K; a.M = M; a.N = N; a.K = K / ksplit;
  a.out = parts; a.ldo = N; a.ntok = 1; a.ksplit = ksplit; a.split_stride = (int64_t)M * N;
  KCHK(launch_gemm(a, EPI_F32, variant, (hipStream_t)stream));
  return JAT_OK;
}
extern "C" int jat_k_gemm_wave_n(int32_t variant) { return gemm_variant(variant) ? gemm_variant(variant)->wave_n() : 0; }
// what the forward launches for a GEMM [M, N, K] at a call site (pinned by tests/golden/gemm_plan.json): the per-decision plans
// where N is the width the site has in the model, a plain GEMM otherwise
extern "C" int jat_k_gemm_plan(const jat_model* m, int32_t site, int32_t M, int32_t N, int32_t K, int32_t folding, int32_t* variant,
                               int32_t* ksplit) {
  if (!m || !variant || !ksplit || site < 0 || site > G_OTHER || M <= 0 || N <= 0 || K <= 0 || K % 64 != 0) return fail(JAT_E_INVALID, "bad argument");
  const bool f = folding != 0, ws = split_ws_slices(M) > 0;
  const GemmPlan p = site == G_QKV && N == m->D + 2 * m->kvD         ? plan_qkv(m, M, K, f, ws)
                     : (site == G_OUT || site == G_FC2) && N == m->D ? plan_resid(m, site, M, K, f, ws)
                     : site == G_OTHER && N == m->bott               ? plan_patch(m, M, K)
                                                                     : plan_gemm(m, site, M, N, 1, f);
  *variant = p.variant; *ksplit = p.ksplit;
  return JAT_OK;
}
extern "C" int jat_k_gemm_fold(const uint16_t* A, const uint16_t* W, const float* bias, void* C, int32_t M, int32_t N, int32_t K,
                               int32_t epilogue, const float* gate, int64_t gate_bstride, int32_t rows_per_batch, uint16_t* hi,
                               uint16_t* lo, float* part_out, const float* part_in, int32_t part_in_np, int32_t variant,
                               void* stream) {
  if (epilogue < 0 || epilogue > EPI_RESID) return fail(JAT_E_INVALID, "epilogue must be 0..3");
  const GemmVariant* t = gemm_variant(variant);
  if (!t || !t->coalesced()) return fail(JAT_E_INVALID, "needs a coalesced-epilogue variant");
  if (hi && (epilogue != EPI_F32 && epilogue != EPI_RESID)) return fail(JAT_E_INVALID, "producer epilogue must be 0 or 3");
  if (hi && (!lo || !part_out)) return fail(JAT_E_INVALID, "producer needs hi, lo and part_out");
  if (part_in && part_in_np != 4 && part_in_np != 8 && part_in_np != 16) return fail(JAT_E_INVALID, "part_in_np must be 4, 8 or 16");
  GemmArgs a{};
  a.A = A; a.W = W; a.lda = K; a.ldw = K; a.M = M; a.N = N; a.K = K;
  a.out = C; a.ldo = N; a.bias = bias; a.gate = gate; a.gate_bstride = gate_bstride;
  a.ntok = rows_per_batch > 0 ? rows_per_batch : 1;
  a.fold_out = hi; a.fold_lo = lo; a.fold_part = part_out;
  if (hi) a.fold_np = N / t->wave_n();
  a.rs_part = part_in; a.rs_np = part_in_np;
  a.dbg_out = timeline_out();
  KCHK(launch_gemm(a, epilogue, variant, (hipStream_t)stream));
  return JAT_OK;
}
// The CFG sampler's step tail on caller buffers: final Linear [M = 2 B ntok, N = 4 C, K] of A = [cond ; uncond] + CFG combine + Euler
// step + next step's patch operand.  fused != 0: one EPI_CFG_EULER launch on the latent in patch layout (z = zp [M/2, N], updated in
// place; xpred unused).  fused == 0: the composition it replaces — EPI_UNPATCH into xpred [2B, C, T = 4 ntok], cfg_euler on
// z [B, C, T], patchify of z — so that a test can compare the two bit for bit.
extern "C" int jat_k_gemm_cfg_euler(const uint16_t* A, const uint16_t* W, const float* bias, int32_t M, int32_t N, int32_t K,
                                    int32_t rows_per_batch, const float* part_in, int32_t part_in_np, float* z, uint16_t* a_patch,
                                    float* xpred, const int32_t* frames, float cfg_scale, float t, float dt, int32_t variant,
                                    int32_t fused, void* stream) {
  if (!A || !W || !z || !a_patch || M <= 0 || M % 2 != 0 || N % 128 != 0 || K % 64 != 0 || rows_per_batch <= 0 ||
      (M / 2) % rows_per_batch != 0)
    return fail(JAT_E_INVALID, "bad argument");
  if (part_in && part_in_np != 4 && part_in_np != 8 && part_in_np != 16) return fail(JAT_E_INVALID, "part_in_np must be 4, 8 or 16");
  if (fused ? !gemm_cfg_euler_supported(variant) : (!gemm_variant(variant) || !xpred))
    return fail(JAT_E_INVALID, fused ? "variant has no CFG + Euler epilogue" : "unknown variant or no xpred");
  hipStream_t s = (hipStream_t)stream;
  const int ntok = rows_per_batch, B = M / 2 / ntok, C = N / 4, T = ntok * 4;
  GemmArgs a{};
  a.A = A; a.W = W; a.lda = K; a.ldw = K; a.M = M; a.N = N; a.K = K; a.bias = bias; a.ntok = ntok;
  a.rs_part = part_in; a.rs_np = part_in_np;
  if (fused) {
    a.out = z; a.ldo = N; a.ce_patch = a_patch; a.ce_frames = frames;
    a.ce_scale = cfg_scale; a.ce_denom = 1.0f - t + 1e-5f; a.ce_dt = dt; a.ce_direct = !(t < 0.999f);
    KCHK(launch_gemm(a, EPI_CFG_EULER, variant, s));
    return JAT_OK;
  }
  a.out = xpred; a.C_out = C; a.T_orig = T;
  KCHK(launch_gemm(a, EPI_UNPATCH, variant, s));
  KCHK(launch_cfg_euler(xpred, z, cfg_scale, t, dt, 1, (int64_t)B * C * T, s));
  KCHK(launch_patchify(z, nullptr, a_patch, B, B, B, C, 0, T, ntok, s, frames));
  return JAT_OK;
}
// The same for one stage of a two-stage solver (EPI_CFG_STAGE; jat_cfg_euler.h): z_base in the layout z has.  fused == 0:
// EPI_UNPATCH into xpred, cfg_stage_kernel on z / z_base [B, C, T], patchify of z.
extern "C" int jat_k_gemm_cfg_stage(const uint16_t* A, const uint16_t* W, const float* bias, int32_t M, int32_t N, int32_t K,
                                    int32_t rows_per_batch, const float* part_in, int32_t part_in_np, float* z, float* z_base,
                                    uint16_t* a_patch, float* xpred, const int32_t* frames, float cfg_scale, float t, float a,
                                    float b, float c, int32_t save, int32_t variant, int32_t fused, void* stream) {
  if (!A || !W || !z || !z_base || !a_patch || M <= 0 || M % 2 != 0 || N % 128 != 0 || K % 64 != 0 || rows_per_batch <= 0 ||
      (M / 2) % rows_per_batch != 0)
    return fail(JAT_E_INVALID, "bad argument");
  if (part_in && part_in_np != 4 && part_in_np != 8 && part_in_np != 16) return fail(JAT_E_INVALID, "part_in_np must be 4, 8 or 16");
  if (fused ? !gemm_cfg_euler_supported(variant) : (!gemm_variant(variant) || !xpred))
    return fail(JAT_E_INVALID, fused ? "variant has no solver-stage epilogue" : "unknown variant or no xpred");
  hipStream_t s = (hipStream_t)stream;
  const int ntok = rows_per_batch, B = M / 2 / ntok, C = N / 4, T = ntok * 4;
  const float den = 1.0f - t + 1e-5f;
  GemmArgs g{};
  g.A = A; g.W = W; g.lda = K; g.ldw = K; g.M = M; g.N = N; g.K = K; g.bias = bias; g.ntok = ntok;
  g.rs_part = part_in; g.rs_np = part_in_np;
  if (fused) {
    g.out = z; g.ldo = N; g.ce_patch = a_patch; g.ce_frames = frames;
    g.ce_scale = cfg_scale; g.ce_denom = den; g.ce_dt = c; g.cs_base = z_base; g.cs_a = a; g.cs_b = b; g.cs_save = save ? 1 : 0;
    KCHK(launch_gemm(g, EPI_CFG_STAGE, variant, s));
    return JAT_OK;
  }
  g.out = xpred; g.C_out = C; g.T_orig = T;
  KCHK(launch_gemm(g, EPI_UNPATCH, variant, s));
  KCHK(launch_cfg_stage(xpred, z, z_base, cfg_scale, den, a, b, c, 1, save ? 1 : 0, (int64_t)B * C * T, s));
  KCHK(launch_patchify(z, nullptr, a_patch, B, B, B, C, 0, T, ntok, s, frames));
  return JAT_OK;
}
// per-kernel entry point (unit parity, tools/tl_probe.py): fused QKV projection + RoPE + GQA attention of 128-token samples,
// W = group-major fused weight [Hkv][5*64 + 64 + 64][K] (q / k rows pair-interleaved per head), out = attention output [M, Hkv*320]
extern "C" int jat_k_qkv_attn(const uint16_t* A, const uint16_t* Wg, const float* bias, uint16_t* out, int32_t M, int32_t Hkv,
                              int32_t K, const float* rope_inv_freq, const float* part_in, int32_t part_in_np, void* stream) {
  if (!A || !Wg || !out || !rope_inv_freq || M <= 0 || M % 128 != 0 || K % 64 != 0) return fail(JAT_E_INVALID, "bad argument");
  GemmArgs a{};
  a.A = A; a.lda = K; a.W = Wg; a.ldw = K; a.M = M; a.N = Hkv * 448; a.K = K;
  a.out = out; a.ldo = (int64_t)Hkv * 320; a.ntok = 128; a.rope_inv_freq = rope_inv_freq; a.bias = bias;
  a.attn_scale_log2e = kAttnScaleLog2e;
  a.rs_part = part_in; a.rs_np = part_in_np;
  a.dbg_out = timeline_out();
  KCHK(launch_qkv_attn(a, (hipStream_t)stream));
  return JAT_OK;
}
extern "C" int jat_k_attention(const uint16_t* q, const uint16_t* k, const uint16_t* vt, uint16_t* o, int32_t B,
                               int32_t N, int32_t Hq, int32_t Hkv, int32_t Npad, void* stream) {
  AttnArgs a{};
  a.q = q; a.k = k; a.vt = vt; a.o = o; a.ldq = (int64_t)Hq * 64; a.ldk = (int64_t)Hkv * 64; a.ldo = (int64_t)Hq * 64;
  a.B = B; a.N = N; a.Hq = Hq; a.Hkv = Hkv; a.npad = Npad;
  a.scale_log2e = kAttnScaleLog2e;
  KCHK(launch_attention(a, (hipStream_t)stream));
  return JAT_OK;
}
// jat_k_attention with per-sample key counts (AttnArgs::lens, as Sampler.run(lengths=...) sets it): same launch_attention
extern "C" int jat_k_attention_lens(const uint16_t* q, const uint16_t* k, const uint16_t* vt, uint16_t* o, const int32_t* lens,
                                    int32_t B, int32_t N, int32_t Hq, int32_t Hkv, int32_t Npad, void* stream) {
  if (!lens) return fail(JAT_E_INVALID, "null lens");
  AttnArgs a{};
  a.q = q; a.k = k; a.vt = vt; a.o = o; a.ldq = (int64_t)Hq * 64; a.ldk = (int64_t)Hkv * 64; a.ldo = (int64_t)Hq * 64;
  a.B = B; a.N = N; a.Hq = Hq; a.Hkv = Hkv; a.npad = Npad;
  a.scale_log2e = kAttnScaleLog2e; a.lens = lens;
  KCHK(launch_attention(a, (hipStream_t)stream));
  return JAT_OK;
}
// which kernel launch_attention starts for this shape (attention.hip); host only, launches nothing
extern "C" int jat_k_attention_route(int32_t N, int32_t Npad, int32_t has_lse, int32_t has_dropout, int32_t* group, int32_t* qt,
                                     int32_t* kvb) {
  if (!group || !qt || !kvb) return fail(JAT_E_INVALID, "null output");
  if (N <= 0 || Npad % 64 != 0 || Npad < N) return fail(JAT_E_INVALID, "N > 0 and Npad a multiple of 64, >= N");
  const AttnRoute r = attention_route(N, Npad, has_lse != 0, has_dropout != 0);
  *group = r.group ? 1 : 0; *qt = r.qt; *kvb = r.kvb;
  return JAT_OK;
}
extern "C" int jat_prof_gemm_site(jat_model* m, int32_t site, int32_t max_launches) {
  if (!m) return fail(JAT_E_INVALID, "null model");
  if (site < -1 || site > G_OTHER) return fail(JAT_E_INVALID, "site must be -1 (off) or 0..4");
  m->prof.site = site; m->prof.n = 0; m->prof.flops = 0.0; m->prof.variant = -1;
  while ((int)m->prof.ev.size() < 2 * max_launches) {
    hipEvent_t e;
    HIPCHK(hipEventCreate(&e));
    m->prof.ev.push_back(e);
  }
  return JAT_OK;
}
extern "C" int jat_prof_collect(jat_model* m, double* total_ms, int32_t* launches, double* flops, int32_t* variant) {
  if (!m) return fail(JAT_E_INVALID, "null model");
  double tot = 0.0;
  for (int i = 0; i < m->prof.n; ++i) {
    HIPCHK(hipEventSynchronize(m->prof.ev[2 * i + 1]));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, m->prof.ev[2 * i], m->prof.ev[2 * i + 1]));
    tot += ms;
  }
  // calibrate: an EMPTY event pair on the same stream measures the marker-to-marker overhead the bracket adds to
  // every launch; subtract it so that the mean agrees with the rocprofv3 kernel-trace duration
  if (m->prof.n > 0 && m->prof.ev.size() >= 2) {
    double ovh = 0.0;
    const int reps = 32;
    for (int i = 0; i < reps; ++i) {
      HIPCHK(hipEventRecord(m->prof.ev[0], m->prof.stream));
      HIPCHK(hipEventRecord(m->prof.ev[1], m->prof.stream));
      HIPCHK(hipEventSynchronize(m->prof.ev[1]));
      float ms = 0.f;
      HIPCHK(hipEventElapsedTime(&ms, m->prof.ev[0], m->prof.ev[1]));
      ovh += ms;
    }
    tot -= ovh / reps * m->prof.n;
    if (tot < 0.0) tot = 0.0;
  }
  if (total_ms) *total_ms = tot;
  if (launches) *launches = m->prof.n;
  if (flops) *flops = m->prof.flops;
  if (variant) *variant = m->prof.variant;
  m->prof.site = -1;
  return JAT_OK;
}
extern "C" int jat_k_cast_bf16(const float* in, uint16_t* out, int64_t n, void* stream) {
  KCHK(launch_cast_bf16(in, out, n, (hipStream_t)stream));
  return JAT_OK;
}
