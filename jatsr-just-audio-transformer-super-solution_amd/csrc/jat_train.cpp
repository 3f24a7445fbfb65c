// Training step of the DiT: the body of train_ddp_v3m2.py:533-622 split at its only
// cross-device boundary.  jat_trainer_fwd_bwd = model(z_t, t, cond) -> mse_loss -> backward into a flat fp32 gradient
// buffer; the caller all-reduces that buffer (RCCL) when world_size > 1; jat_trainer_optim = clip_grad_norm_ + AdamW +
// re-pack of the bf16 operand copies.  Sequencing only: the arithmetic lives in gemm.hip / attention.hip /
// elementwise.hip / train.hip.
//
// Every Linear runs its forward and input-gradient GEMMs on gemm_bf16_kernel (C = A W^T, both operands K-contiguous) and its
// weight gradient on gemm_tn.hip, straight from the token-major operands:
//   y  = x  W^T        A = x [M,in]          W = W   [out,in]
//   dx = dy W          A = dy [M,out]        W = W^T [in,out]     (transposed bf16 copy, rebuilt after every update)
//   dW = dy^T x        jat_weight_grad below
#include <algorithm>
#include <array>
#include <cstdlib>
#include <string>
#include <unordered_map>
#include <vector>

#include "jat_internal.h"

namespace {

struct TLayer {
  float *x_mid, *lse;
  bf16_t *xn1, *q, *k, *vt, *ao, *y_attn, *xn2, *h_pre, *h_post, *y_mlp;
  bf16_t *wqkvT, *woT, *w1T, *w2T;
  int64_t off[P_COUNT];   // by ParamId: where this block's parameters (and their gradients) start in the flat buffers, in floats
};

}  // namespace

struct jat_trainer {
  jat_model* m = nullptr;
  int B = 0, T = 0, ntok = 0, M = 0, npad = 0;
  float *P = nullptr, *G = nullptr, *m1 = nullptr, *m2 = nullptr;
  float* ema = nullptr;                // caller-owned moving average of P (jat_trainer_set_ema); nullptr: off
  float ema_decay = 0.f;
  int64_t total = 0;
  char* blob = nullptr;
  size_t blob_bytes = 0;
  std::vector<float*> x;               // depth + 1 residual-stream snapshots [M, D]
  std::vector<TLayer> L;
  bf16_t *a_patch, *pe_pre, *pe_h, *xnf, *t_silu, *pe_w2T, *wfinalT;
  float *e_sin, *u1, *t_h, *t_emb, *mod, *pred;
  // backward scratch
  float *dx, *dpred, *dmod, *part, *red_part, *scal, *delta, *dwqkv, *dt_emb, *du1, *small_part;
  bf16_t *dy, *dh, *dxn, *dao, *dqkv, *dyf;
  int64_t off[P_COUNT];                // by ParamId: the head's and the final layer's parameters in the flat buffers (floats)
  int64_t& offset_of(const ParamDesc& e) { return (e.block >= 0 && e.block < (int)L.size() ? L[e.block].off : off)[e.id]; }
  bool rms = true;
  // gradient-ready hook (DDP overlap): called on the host, during enqueue, once the last kernel writing the slice
  // grads_flat[off, off + n) has been enqueued — final layer first, then blocks depth-1 .. 0, then patch embed + t_embedder
  void (*hook)(int64_t off, int64_t n, void* user) = nullptr;
  void* hook_user = nullptr;
  std::vector<int64_t> block_lo;       // first float of block l's parameters (depth + 1 entries: [depth] = final layer)
  std::vector<float> p_drop, p_path;   // per-layer Dropout / DropPath rates (jat_trainer_set_regularisers); default 0
  uint64_t seed = 0;                   // RNG seed of the step in flight (masks are recomputed by the backward)
  CopyJob* copy_jobs = nullptr;        // device table: fp32 master slices -> the model's fp32 operand tensors
  int n_copy_jobs = 0;
  float* dw_part = nullptr;
  LossSpec loss;                       // the three jat_trainer_set_* loss setters; default: plain MSE (the V3 trainer)
  float2* tw = nullptr;                // [T] twiddles
  float *ll_part = nullptr, *terms = nullptr;
  float* dw_split = nullptr;           // split-K partial slices of the dW GEMMs
  const void* zero_cell = nullptr;     // 256 zero bytes (the workspace is zeroed once and this cell is never written)
  float* colsum_part = nullptr;        // row-slice partials of the bias-gradient column sums
  float* dkv_part = nullptr;           // per-query-head fp32 partials of dK / dV (attention backward)
  // Weight gradients on a second stream (JAT_DW_STREAM=1).  dW = dY^T X of a Linear is off the critical path of the backward (nothing
  // reads it before the gradient norm), while the dX chain in front of it alternates MFMA-bound GEMMs with HBM- / VALU-bound
  // passes (norm and gate backward, GELU', attention backward): with the dW GEMMs queued beside that chain the chip works on a
  // GEMM while the chain is in a memory pass.  The four gradient operands a layer hands to its dW GEMMs (dy of the MLP branch,
  // dh, dy of the attention branch, dqkv) are double-buffered by layer parity, so the chain runs up to one layer ahead of the dW
  // stream; events order producer -> dW (ready) and dW -> next writer of the same buffer (done).
  bool dw_async = false;
  hipStream_t dw_stream = nullptr;
  hipEvent_t ev_ready[4][2] = {}, ev_done[4][2] = {}, ev_mod[2] = {}, ev_join = nullptr, ev_wt = nullptr;
  std::vector<hipEvent_t> ev_layer;    // block l's weight gradients are complete (gates the gradient-ready hook)
  bf16_t *dy_m[2] = {}, *dh_b[2] = {}, *dy_a[2] = {}, *dq_b[2] = {};
  // the call in flight (jat_trainer_fwd_bwd_ex flags): accum: every writer of grads_flat, and the loss cells, add to what is there;
  // no_hook: the gradient-ready hook stays silent (not the last micro-batch of the optimiser step)
  bool accum = false, no_hook = false;

  // whatever jat_trainer_create got as far as making: the second stream (drained first: its work reads the workspace), the events,
  // the workspace
  ~jat_trainer() {
    if (dw_stream) { (void)hipStreamSynchronize(dw_stream); (void)hipStreamDestroy(dw_stream); }
    auto drop = [](hipEvent_t e) { if (e) (void)hipEventDestroy(e); };
    for (int k = 0; k < 4; ++k)
      for (int q = 0; q < 2; ++q) { drop(ev_ready[k][q]); drop(ev_done[k][q]); }
    for (hipEvent_t e : {ev_join, ev_wt, ev_mod[0], ev_mod[1]}) drop(e);
    for (hipEvent_t e : ev_layer) drop(e);
    if (blob) (void)hipFree(blob);
  }
};

namespace {

int build_transposes(jat_trainer* tr, hipStream_t s) {
  jat_model* m = tr->m;
  const int D = m->D, Nqkv = D + 2 * m->kvD;
  for (int l = 0; l < m->depth; ++l) {
    const LayerW& W = m->layers[l];
    TLayer& L = tr->L[l];
    KCHK(launch_transpose_bf16(W.wqkv, D, Nqkv, D, L.wqkvT, Nqkv, s));
    KCHK(launch_transpose_bf16(W.wo, D, D, D, L.woT, D, s));
    KCHK(launch_transpose_bf16(W.w1, D, m->mlp, D, L.w1T, m->mlp, s));
    KCHK(launch_transpose_bf16(W.w2, m->mlp, D, m->mlp, L.w2T, D, s));
  }
  KCHK(launch_transpose_bf16(m->pe_w2, m->bott, D, m->bott, tr->pe_w2T, D, s));
  KCHK(launch_transpose_bf16(m->wfinal, D, m->Fout, D, tr->wfinalT, m->Fout, s));
  return JAT_OK;
}

// After an optimiser step: fp32 master -> the operand copies the kernels read.  No host synchronisation; the small
// fp32 tensors go in one table-driven launch, the GEMM weights in one cast per matrix, then the transposed copies.
// The group-major QKV copy of the fused inference kernel is NOT rebuilt (m->group_copy_stale).
int repack(jat_trainer* tr, hipStream_t s) {
  jat_model* m = tr->m;
  m->group_copy_stale = true;
  m->fold_src_ok = false;    // the sampler's folded-weight tables (jat_api.cpp FoldTable) describe the previous weights:
  m->fold_cache.clear();     // samplers created from now on run the norm kernels until the next full load
  KCHK(launch_multi_copy(tr->copy_jobs, tr->n_copy_jobs, s));   // the fp32 parameters
  for (const ParamDesc& e : m->params) {
    if (e.form == F_F32) continue;
    const float* src = tr->P + tr->offset_of(e);
    if (e.form == F_BF16_ROPE) KCHK(launch_cast_bf16_rope_rows(src, m->at<bf16_t>(e), e.rows, e.cols, s));
    else KCHK(launch_cast_bf16(src, m->at<bf16_t>(e), e.numel(), s));
  }
  if (tr->dw_async) {
    // the transposed copies are read by the NEXT backward only (dX = dY W): rebuilt on the second stream, under the next forward
    // (HBM-bound copies beside MFMA-bound GEMMs); backward_train waits for ev_wt before its first dX GEMM
    HIPCHK(hipEventRecord(tr->ev_join, s));
    HIPCHK(hipStreamWaitEvent(tr->dw_stream, tr->ev_join, 0));
    JCHK(build_transposes(tr, tr->dw_stream));
    HIPCHK(hipEventRecord(tr->ev_wt, tr->dw_stream));
    return JAT_OK;
  }
  return build_transposes(tr, s);
}

// The weights whose gradient is a [out, in] GEMM over all tokens (weight_grad below), as {out, in}: final Linear, MLP fc2 / fc1,
// out_proj, fused QKV, patch-embed proj.2 / proj.0
std::array<std::array<int, 2>, 7> dw_shapes(const jat_model* m) {
  const int D = m->D;
  return {{{m->Fout, D}, {D, m->mlp}, {m->mlp, D}, {D, D}, {D + 2 * m->kvD, D}, {D, m->bott}, {m->bott, m->Kp}}};
}

// dW[out,in] = dY^T X and (optionally) db[out] = column sums of dY, from dY bf16 [M,out] and X bf16 [M,in]; acc: added into
// dW / db (G = G_old + g) instead of overwriting them
int weight_grad(jat_trainer* tr, const bf16_t* dY, int out, const bf16_t* X, int in, float* dW, float* db, bool acc, hipStream_t s) {
  return jat_weight_grad(dY, X, dW, db, tr->M, out, in, gemm_tn_ksplit(out, in, tr->M), tr->zero_cell, tr->dw_split, tr->colsum_part,
                         acc, s);
}

// dX bf16 [M,in] = dY [M,out] W, with WT = W^T [in,out]
int input_grad(jat_trainer* tr, const bf16_t* dY, int out, const bf16_t* WT, int in, bf16_t* dX, hipStream_t s) {
  GemmArgs e{};
  e.out = dX; e.ldo = in; e.ntok = tr->ntok;
  return jat_gemm(tr->m, G_OTHER, dY, out, WT, out, tr->M, in, out, EPI_BF16, e, s);
}

// mask sites of layer l (jat_rng.h): 0 attention probabilities, 1 DropPath(attn), 2 MLP after GELU, 3 MLP out, 4 DropPath(MLP)
DropSpec site(const jat_trainer* tr, int l, int kind) {
  const float p = (kind == 1 || kind == 4) ? tr->p_path[l] : tr->p_drop[l];
  return jat_drop_spec(tr->seed, (uint32_t)(l * 8 + kind), p);
}
const DropSpec kNoDrop = {0u, 0u, 0u, 1.0f};

int forward_train(jat_trainer* tr, const float* z_t, const float* t, const float* x_cond, hipStream_t s) {
  jat_model* m = tr->m;
  const int B = tr->B, T = tr->T, ntok = tr->ntok, M = tr->M, D = m->D, Nqkv = D + 2 * m->kvD;
  const int64_t mstride = (int64_t)m->depth * 6 * D;
  // t_embedder (fp32; jat_audiosr_v3.py:364-369) with the pre-activation kept for the backward
  KCHK(launch_time_sinusoid(t, tr->e_sin, B, D, s));
  KCHK(launch_linear_f32(tr->e_sin, m->te_w1, m->te_b1, tr->u1, nullptr, B, D, D, 0, s));
  KCHK(launch_silu_f32(tr->u1, tr->t_h, (int64_t)B * D, s));
  KCHK(launch_linear_f32(tr->t_h, m->te_w2, m->te_b2, tr->t_emb, tr->t_silu, B, D, D, 0, s));
  {
    GemmArgs e{};
    e.out = tr->mod; e.ldo = mstride; e.bias = m->bada; e.ntok = 1;
    JCHK(jat_gemm(m, G_OTHER, tr->t_silu, D, m->wada, D, B, (int)mstride, D, EPI_F32, e, s));
  }
  KCHK(launch_patchify(z_t, x_cond, tr->a_patch, B, B, B, m->Cin, m->Cc, T, ntok, s));
  {
    GemmArgs e{};
    e.out = tr->pe_pre; e.ldo = m->bott; e.bias = m->pe_b1; e.ntok = ntok;
    JCHK(jat_gemm(m, G_OTHER, tr->a_patch, m->Kp, m->pe_w1, m->Kp, M, m->bott, m->Kp, EPI_BF16, e, s));
    KCHK(launch_gelu_bf16(tr->pe_pre, tr->pe_h, (int64_t)M * m->bott, kNoDrop, s));
    GemmArgs f{};
    f.out = tr->x[0]; f.ldo = D; f.bias = m->pe_b2; f.ntok = ntok;
    JCHK(jat_gemm(m, G_OTHER, tr->pe_h, m->bott, m->pe_w2, m->bott, M, D, m->bott, EPI_F32, f, s));
  }
  for (int l = 0; l < m->depth; ++l) {
    const LayerW& W = m->layers[l];
    TLayer& L = tr->L[l];
    const float* mod = tr->mod + (int64_t)l * 6 * D;
    KCHK(launch_norm_modulate(tr->x[l], W.norm1, mod + 0 * D, mod + 1 * D, mstride, L.xn1, M, D, ntok, m->cfg.norm_mode, s));
    {
      GemmArgs e{};
      e.out = L.q; e.k_out = L.k; e.vt_out = L.vt; e.D = D; e.kvD = m->kvD; e.npad = tr->npad; e.ntok = ntok;
      e.rope_cos = m->rope_cos; e.rope_sin = m->rope_sin; e.rope_inv_freq = m->rope_invf;
      JCHK(jat_gemm(m, G_QKV, L.xn1, D, W.wqkv, D, M, Nqkv, D, EPI_QKV_ROPE, e, s));
    }
    {
      AttnArgs a{};
      a.q = L.q; a.k = L.k; a.vt = L.vt; a.o = L.ao; a.ldq = D; a.ldk = m->kvD; a.ldo = D;
      a.B = B; a.N = ntok; a.Hq = m->Hq; a.Hkv = m->Hkv; a.npad = tr->npad;
      a.scale_log2e = 0.125f * 1.4426950408889634f;
      a.lse = L.lse;
      a.drop = site(tr, l, 0);
      KCHK(launch_attention(a, s));
    }
    {
      GemmArgs e{};
      e.out = L.y_attn; e.ldo = D; e.ntok = ntok;
      JCHK(jat_gemm(m, G_OUT, L.ao, D, W.wo, D, M, D, D, EPI_BF16, e, s));
    }
    KCHK(launch_resid_gate(tr->x[l], L.y_attn, mod + 2 * D, mstride, L.x_mid, M, D, ntok, site(tr, l, 1), kNoDrop, s));
    KCHK(launch_norm_modulate(L.x_mid, W.norm2, mod + 3 * D, mod + 4 * D, mstride, L.xn2, M, D, ntok, m->cfg.norm_mode, s));
    {
      GemmArgs e{};
      e.out = L.h_pre; e.ldo = m->mlp; e.bias = W.b1; e.ntok = ntok;
      JCHK(jat_gemm(m, G_FC1, L.xn2, D, W.w1, D, M, m->mlp, D, EPI_BF16, e, s));
      KCHK(launch_gelu_bf16(L.h_pre, L.h_post, (int64_t)M * m->mlp, site(tr, l, 2), s));
      GemmArgs f{};
      f.out = L.y_mlp; f.ldo = D; f.bias = W.b2; f.ntok = ntok;
      JCHK(jat_gemm(m, G_FC2, L.h_post, m->mlp, W.w2, m->mlp, M, D, m->mlp, EPI_BF16, f, s));
    }
    KCHK(launch_resid_gate(L.x_mid, L.y_mlp, mod + 5 * D, mstride, tr->x[l + 1], M, D, ntok, site(tr, l, 4), site(tr, l, 3), s));
  }
  KCHK(launch_norm_modulate(tr->x[m->depth], m->final_norm, nullptr, nullptr, 0, tr->xnf, M, D, ntok, m->cfg.norm_mode, s));
  {
    GemmArgs e{};
    e.out = tr->pred; e.bias = m->bfinal; e.ntok = ntok; e.C_out = m->Cin; e.T_orig = T;
    JCHK(jat_gemm(m, G_OTHER, tr->xnf, D, m->wfinal, D, M, m->Fout, D, EPI_UNPATCH, e, s));
  }
  return JAT_OK;
}

int backward_train(jat_trainer* tr, const float* target, const float* cond_clean, float loss_scale, hipStream_t s) {
  jat_model* m = tr->m;
  const int B = tr->B, T = tr->T, ntok = tr->ntok, M = tr->M, D = m->D, Nqkv = D + 2 * m->kvD, mode = m->cfg.norm_mode;
  const int64_t mstride = (int64_t)m->depth * 6 * D;
  float* G = tr->G;
  const bool acc = tr->accum;
  // the loss cells add up as the gradients do: kept aside here, added back in behind the loss kernels
  // the loss lands in scal[0]; a loss with a latent term writes its six terms and their total is copied there
  float *terms = tr->loss.has_latent() ? tr->terms : nullptr, *terms_keep = terms ? terms + 8 : nullptr;
  if (acc) KCHK(launch_loss_carry(tr->scal, tr->scal + 12, terms, terms_keep, 0, s));
  JCHK(run_loss(tr->loss, plan_loss(tr->loss, B * m->Cin, T), tr->pred, target, cond_clean, tr->tw, tr->dpred,
                terms ? tr->ll_part : tr->red_part, terms ? terms : tr->scal, B * m->Cin, T, loss_scale, s));
  if (terms) HIPCHK(hipMemcpyAsync(tr->scal, terms, 4, hipMemcpyDeviceToDevice, s));
  if (acc) KCHK(launch_loss_carry(tr->scal, tr->scal + 12, terms, terms_keep, 1, s));
  // Where a weight gradient runs: on `s` itself, or (dw_async) on the second stream behind an event of the kernel that
  // finished its gradient operand; `done` is what the next writer of that operand buffer waits for.
  hipStream_t ws = tr->dw_async ? tr->dw_stream : s;
  auto dw_begin = [&](hipEvent_t ready) -> int {
    if (!tr->dw_async) return JAT_OK;
    HIPCHK(hipEventRecord(ready, s));
    HIPCHK(hipStreamWaitEvent(ws, ready, 0));
    return JAT_OK;
  };
  auto dw_end = [&](hipEvent_t done) -> int {
    if (tr->dw_async) HIPCHK(hipEventRecord(done, ws));
    return JAT_OK;
  };
  auto before_write = [&](hipEvent_t done) -> int {   // a never-recorded event does not block
    if (tr->dw_async) HIPCHK(hipStreamWaitEvent(s, done, 0));
    return JAT_OK;
  };
  // gradient-ready hook of a block: with the second stream its weight gradients may still be in flight when the chain moves on,
  // so the hook of block l fires one block later, behind an event of the dW stream (the exchange stream orders itself after `s`)
  int pending_hook = -1;
  auto fire_hook = [&](int blk) -> int {
    if (!tr->hook || tr->no_hook) return JAT_OK;
    if (tr->dw_async) HIPCHK(hipStreamWaitEvent(s, tr->ev_layer[blk], 0));
    tr->hook(tr->block_lo[blk], (blk == m->depth ? tr->total : tr->block_lo[blk + 1]) - tr->block_lo[blk], tr->hook_user);
    return JAT_OK;
  };
  // everything that queues work on the second stream, so that a failure in the middle still reaches the join below
  auto chain = [&]() -> int {
    // final layer: Linear (unpatchify^T is a patchify of dpred) and the un-modulated norm
    KCHK(launch_patchify(tr->dpred, nullptr, tr->dyf, B, B, B, m->Cin, 0, T, ntok, s));
    if (tr->dw_async) HIPCHK(hipStreamWaitEvent(s, tr->ev_wt, 0));   // the transposed weight copies of the last re-pack (repack())
    JCHK(input_grad(tr, tr->dyf, m->Fout, tr->wfinalT, D, tr->dxn, s));
    if (tr->dw_async) { HIPCHK(hipEventRecord(tr->ev_join, s)); HIPCHK(hipStreamWaitEvent(ws, tr->ev_join, 0)); }
    JCHK(weight_grad(tr, tr->dyf, m->Fout, tr->xnf, D, G + tr->off[P_WF], G + tr->off[P_BF], acc, ws));
    if (tr->dw_async) HIPCHK(hipEventRecord(tr->ev_layer[m->depth], ws));
    KCHK(launch_norm_bwd(tr->x[m->depth], tr->dxn, m->final_norm, nullptr, 0, tr->dx, 0, tr->part, tr->dw_part, nullptr, nullptr, 0,
                         tr->rms ? G + tr->off[P_FN] : nullptr, acc, B, D, ntok, mode, s));
    if (tr->dw_async) pending_hook = m->depth; else JCHK(fire_hook(m->depth));
    for (int l = m->depth - 1; l >= 0; --l) {
      TLayer& L = tr->L[l];
      const int par = l & 1;
      bf16_t *dy_m = tr->dy_m[par], *dh = tr->dh_b[par], *dy_a = tr->dy_a[par], *dq = tr->dq_b[par];
      const float* mod = tr->mod + (int64_t)l * 6 * D;
      float* dmod = tr->dmod + (int64_t)l * 6 * D;
      // x_out = x_mid + gate_mlp * mlp(norm2(x_mid) * (1 + scale_mlp) + shift_mlp)          jat_audiosr_v3.py:303-306
      JCHK(before_write(tr->ev_done[0][par]));
      KCHK(launch_gate_bwd(tr->dx, L.y_mlp, mod + 5 * D, mstride, dy_m, tr->part, dmod + 5 * D, mstride, B, D, ntok,
                           site(tr, l, 4), site(tr, l, 3), s));
      JCHK(before_write(tr->ev_done[1][par]));
      JCHK(input_grad(tr, dy_m, D, L.w2T, m->mlp, dh, s));
      JCHK(dw_begin(tr->ev_ready[0][par]));
      JCHK(weight_grad(tr, dy_m, D, L.h_post, m->mlp, G + L.off[P_W2], G + L.off[P_B2], acc, ws));
      JCHK(dw_end(tr->ev_done[0][par]));
      KCHK(launch_gelu_bwd(L.h_pre, dh, (int64_t)M * m->mlp, site(tr, l, 2), s));
      JCHK(input_grad(tr, dh, m->mlp, L.w1T, D, tr->dxn, s));
      JCHK(dw_begin(tr->ev_ready[1][par]));
      JCHK(weight_grad(tr, dh, m->mlp, L.xn2, D, G + L.off[P_W1], G + L.off[P_B1], acc, ws));
      JCHK(dw_end(tr->ev_done[1][par]));
      KCHK(launch_norm_bwd(L.x_mid, tr->dxn, m->layers[l].norm2, mod + 4 * D, mstride, tr->dx, 1, tr->part, tr->dw_part, dmod + 3 * D,
                           dmod + 4 * D, mstride, tr->rms ? G + L.off[P_N2] : nullptr, acc, B, D, ntok, mode, s));
      // x_mid = x_in + gate_msa * out_proj(attn(norm1(x_in) * (1 + scale_msa) + shift_msa))   :297-300
      JCHK(before_write(tr->ev_done[2][par]));
      KCHK(launch_gate_bwd(tr->dx, L.y_attn, mod + 2 * D, mstride, dy_a, tr->part, dmod + 2 * D, mstride, B, D, ntok,
                           site(tr, l, 1), kNoDrop, s));
      JCHK(input_grad(tr, dy_a, D, L.woT, D, tr->dao, s));
      JCHK(dw_begin(tr->ev_ready[2][par]));
      JCHK(weight_grad(tr, dy_a, D, L.ao, D, G + L.off[P_O], nullptr, acc, ws));
      JCHK(dw_end(tr->ev_done[2][par]));
      JCHK(before_write(tr->ev_done[3][par]));
      KCHK(launch_attention_bwd(L.q, L.k, L.vt, L.ao, tr->dao, L.lse, tr->delta, dq, m->rope_cos, m->rope_sin, B, ntok,
                                m->Hq, m->Hkv, tr->npad, site(tr, l, 0), tr->dkv_part, s));
      JCHK(input_grad(tr, dq, Nqkv, L.wqkvT, D, tr->dxn, s));
      JCHK(dw_begin(tr->ev_ready[3][par]));
      JCHK(weight_grad(tr, dq, Nqkv, L.xn1, D, tr->dwqkv, nullptr, false, ws));   // scratch: the unpack below is what accumulates
      KCHK(launch_unpack_qkv_grad(tr->dwqkv, G + L.off[P_Q], G + L.off[P_K], G + L.off[P_V], D, m->kvD, D, acc, ws));
      JCHK(dw_end(tr->ev_done[3][par]));
      KCHK(launch_norm_bwd(tr->x[l], tr->dxn, m->layers[l].norm1, mod + 1 * D, mstride, tr->dx, 1, tr->part, tr->dw_part, dmod + 0 * D,
                           dmod + 1 * D, mstride, tr->rms ? G + L.off[P_N1] : nullptr, acc, B, D, ntok, mode, s));
      // adaLN modulation Linear(SiLU(t_emb)) of this block (:275-278): its six dmod slices are complete now (a weight gradient
      // like the others: nothing in the chain reads it)
      JCHK(dw_begin(tr->ev_mod[par]));
      KCHK(launch_small_dw(dmod, mstride, tr->t_emb, D, G + L.off[P_ADA_W], G + L.off[P_ADA_B], B, 6 * D, D, 1, acc, ws));
      if (tr->dw_async) HIPCHK(hipEventRecord(tr->ev_layer[l], ws));
      if (tr->dw_async) {
        if (pending_hook >= 0) JCHK(fire_hook(pending_hook));
        pending_hook = l;
      } else {
        JCHK(fire_hook(l));
      }
    }
    return JAT_OK;
  };
  const int chain_rc = chain();
  // join: everything below (and the optimiser) runs on `s` alone again and may reuse the dW scratch.  Also when the chain failed:
  // whatever it did queue on the second stream is ordered before the caller's next work on `s` — an accumulating call reads
  // the gradients the previous call's second stream wrote.
  if (tr->dw_async) {
    HIPCHK(hipEventRecord(tr->ev_join, ws));
    HIPCHK(hipStreamWaitEvent(s, tr->ev_join, 0));
  }
  if (chain_rc != JAT_OK) return chain_rc;
  if (tr->dw_async && pending_hook >= 0) JCHK(fire_hook(pending_hook));
  // patch embed: Linear(Kp -> bott) - GELU - Linear(bott -> D)   (jat_audiosr_v3.py:221-225); no gradient to the input
  KCHK(launch_cast_bf16(tr->dx, tr->dy, (int64_t)M * D, s));
  JCHK(input_grad(tr, tr->dy, D, tr->pe_w2T, m->bott, tr->dh, s));
  JCHK(weight_grad(tr, tr->dy, D, tr->pe_h, m->bott, G + tr->off[P_PE_W2], G + tr->off[P_PE_B2], acc, s));
  KCHK(launch_gelu_bwd(tr->pe_pre, tr->dh, (int64_t)M * m->bott, kNoDrop, s));
  JCHK(weight_grad(tr, tr->dh, m->bott, tr->a_patch, m->Kp, G + tr->off[P_PE_W1], G + tr->off[P_PE_B1], acc, s));
  // the t_embedder MLP (:364-369) behind all adaLN Linears; fp32, B rows
  // d silu(t_emb) = dmod [B, depth*6D] @ W_ada (the packed bf16 copy the forward multiplied with), all layers at once
  KCHK(launch_small_dx(tr->dmod, mstride, m->wada, 1, tr->small_part, tr->dt_emb, B, (int)mstride, D, 0, tr->t_emb, s));
  KCHK(launch_small_dw(tr->dt_emb, D, tr->t_h, D, G + tr->off[P_TE_W2], G + tr->off[P_TE_B2], B, D, D, 0, acc, s));
  KCHK(launch_small_dx(tr->dt_emb, D, tr->P + tr->off[P_TE_W2], 0, tr->small_part, tr->du1, B, D, D, 0, tr->u1, s));
  KCHK(launch_small_dw(tr->du1, D, tr->e_sin, D, G + tr->off[P_TE_W1], G + tr->off[P_TE_B1], B, D, D, 0, acc, s));
  if (tr->hook && !tr->no_hook) tr->hook(0, tr->block_lo[0], tr->hook_user);
  return JAT_OK;
}

}  // namespace

// ---- one weight gradient (jat_internal.h): the trainer's weight_grad and jat_k_weight_grad_ex both run this ------------
DwScratch jat_weight_grad_scratch(int tokens, int out, int in, int ksplit, bool with_db) {
  return {ksplit > 1 ? (size_t)ksplit * out * in : 0, with_db ? (size_t)colsum_slices(tokens) * out : 0};
}

int jat_weight_grad(const bf16_t* dY, const bf16_t* X, float* dW, float* db, int tokens, int out, int in, int ksplit,
                    const void* zeros, float* split, float* colsum, bool acc, hipStream_t s) {
  // M x N tiles of a small weight do not fill 256 CUs while K = all tokens is long: split K, sum the partials in order
  const int64_t area = (int64_t)out * in;
  // one slice: the add happens in the GEMM's epilogue; several: the slices are overwritten, their ordered sum is added
  KCHK(launch_gemm_tn(dY, out, X, in, ksplit > 1 ? split : dW, in, out, in, tokens, ksplit, area, zeros, acc && ksplit == 1, s));
  if (ksplit > 1) KCHK(launch_sum_partials(split, ksplit, area, dW, area, acc, s));
  if (db) KCHK(launch_colsum_bf16(dY, out, tokens, out, colsum, db, acc, s));
  return JAT_OK;
}

extern "C" void jat_trainer_destroy(jat_trainer* tr) { delete tr; }

extern "C" int jat_trainer_create(jat_model* m, const jat_tensor_ref* params, int32_t n, float* params_flat,
                                  float* grads_flat, float* exp_avg, float* exp_avg_sq, int64_t total, int32_t B,
                                  int32_t T, void* stream, jat_trainer** out) {
  if (!m || !params || !params_flat || !grads_flat || !exp_avg || !exp_avg_sq || !out)
    return fail(JAT_E_INVALID, "null argument");
  if (B <= 0 || T <= 0) return fail(JAT_E_INVALID, "B and T must be positive");
  if (B > 32) return fail(JAT_E_INVALID, "per-rank batch %d > 32 is not supported by the adaLN backward", B);
  // the condition is the LR latent of the HR latent's shape: prepare, the losses and the Python driver take it at input_channels
  if (m->Cc != m->Cin)
    return fail(JAT_E_INVALID, "the trainer conditions on a latent of the target's shape: cond_channels (%d) must equal input_channels (%d)",
                m->Cc, m->Cin);
  if (total <= 0 || total % 4 != 0) return fail(JAT_E_INVALID, "flat buffer length must be a positive multiple of 4");
  const int ntok = (T + 3) / 4;
  if (ntok > MAX_LEN) return fail(JAT_E_SEQLEN, "Sequence length %d exceeds max_len %d", ntok, MAX_LEN);
  hipStream_t s = (hipStream_t)stream;
  auto owner = std::make_unique<jat_trainer>();   // every error return below releases what was created so far
  jat_trainer* tr = owner.get();
  tr->m = m; tr->B = B; tr->T = T; tr->ntok = ntok; tr->M = B * ntok;
  tr->npad = (int)align_up((size_t)ntok, 64);
  tr->P = params_flat; tr->G = grads_flat; tr->m1 = exp_avg; tr->m2 = exp_avg_sq; tr->total = total;
  tr->rms = m->cfg.norm_mode == JAT_NORM_RMS_W;
  tr->p_drop.assign(m->depth, 0.f);
  tr->p_path.assign(m->depth, 0.f);
  const int D = m->D, depth = m->depth, mlp = m->mlp, bott = m->bott, kvD = m->kvD, Nqkv = D + 2 * kvD;
  const int M = tr->M;
  // every weight gradient runs on gemm_tn.hip.  jat_model_create's divisibility rules imply this; a model that broke it would
  // otherwise fail at its first backward launch
  for (auto& sh : dw_shapes(m))
    if (!gemm_tn_supports(sh[0], sh[1]))
      return fail(JAT_E_INVALID, "weight [%d, %d]: the weight-gradient GEMM needs both widths to be multiples of 128", sh[0], sh[1]);

  // ---- parameter table: every tensor must lie inside the flat buffer, 16-B aligned, with the expected size ----
  std::unordered_map<std::string, const jat_tensor_ref*> given;
  for (int i = 0; i < n; ++i) {
    const int64_t o = params[i].data - params_flat;
    if (o < 0 || o + params[i].numel > total || o % 4 != 0)
      return fail(JAT_E_INVALID, "parameter '%s' is not a 16-byte aligned slice of the flat buffer", params[i].name);
    given[params[i].name] = &params[i];
  }
  // every parameter of the model resolved to its offset; per group (head, block l, final layer = block `depth`) the range it
  // covers: block l = [block_lo[l], block_lo[l+1]) is what the gradient-ready hook reports
  int rc = JAT_OK;
  size_t used = 0;
  int64_t head_hi = -1;
  tr->L.resize(depth);
  tr->block_lo.assign(depth + 1, total);
  for (const ParamDesc& e : m->params) {
    if (!m->has(e)) continue;
    auto it = given.find(e.name);
    if (it == given.end()) { rc = fail(JAT_E_STATE, "missing parameter '%s'", e.name.c_str()); break; }
    if (it->second->numel != e.numel()) {
      rc = fail(JAT_E_INVALID, "parameter '%s' has %lld elements, expected %lld", e.name.c_str(), (long long)it->second->numel,
                (long long)e.numel());
      break;
    }
    ++used;
    const int64_t o = tr->offset_of(e) = it->second->data - params_flat;
    if (e.block < 0) head_hi = std::max(head_hi, o);
    else tr->block_lo[e.block] = std::min(tr->block_lo[e.block], o);
  }
  for (int l = 0; l < depth && rc == JAT_OK; ++l)
    if (tr->block_lo[l] >= tr->block_lo[l + 1])
      rc = fail(JAT_E_INVALID, "parameters of block %d are not laid out before those of block %d / the final layer", l, l + 1);
  if (rc == JAT_OK && head_hi >= tr->block_lo[0])
    rc = fail(JAT_E_INVALID, "patch_embed / t_embedder parameters must precede the blocks in the flat buffer");
  if (rc == JAT_OK && used != (size_t)n)
    rc = fail(JAT_E_INVALID, "%d parameters given, %zu belong to this model: every trainable tensor must be known", n, used);
  if (rc != JAT_OK) return rc;

  tr->dw_async = true;   // measured: 61.2 -> 58.5 ms per step at T = 1378, 33.3 -> 31.5 ms at T = 512 (profiles/r03/train_dw_stream_ab.log)
  if (const char* e = getenv("JAT_DW_STREAM")) tr->dw_async = atoi(e) != 0;
  if (tr->dw_async) {
    // lowest priority: when both queues have a GEMM ready, the chain's (critical path) goes first
    int prio_least = 0, prio_greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
    static const int prio_env = getenv("JAT_DW_STREAM_PRIO") ? atoi(getenv("JAT_DW_STREAM_PRIO")) : 1;
    bool ok = (prio_env ? hipStreamCreateWithPriority(&tr->dw_stream, hipStreamNonBlocking, prio_least)
                        : hipStreamCreateWithFlags(&tr->dw_stream, hipStreamNonBlocking)) == hipSuccess;
    auto mk = [&](hipEvent_t* e) { ok = ok && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess; };
    for (int k = 0; k < 4; ++k)
      for (int q = 0; q < 2; ++q) { mk(&tr->ev_ready[k][q]); mk(&tr->ev_done[k][q]); }
    mk(&tr->ev_join); mk(&tr->ev_wt); mk(&tr->ev_mod[0]); mk(&tr->ev_mod[1]);
    tr->ev_layer.assign((size_t)depth + 1, nullptr);
    for (auto& e : tr->ev_layer) mk(&e);
    if (!ok) return fail(JAT_E_HIP, "stream / event creation for the weight-gradient stream failed");
  }
  // ---- one allocation: transposed weights, saved activations, backward scratch ----
  const size_t n_f32 = std::count_if(m->params.begin(), m->params.end(), [](const ParamDesc& e) { return e.form == F_F32; });
  for (int pass = 0; pass < 2; ++pass) {
    size_t o = 0;
    char* base = tr->blob;
    auto take = [&](size_t bytes) { char* p = base ? base + o : nullptr; o += align_up(bytes, 256); return p; };
    const size_t MD2 = (size_t)M * D * 2, MD4 = (size_t)M * D * 4;
    tr->x.resize(depth + 1);
    for (int l = 0; l <= depth; ++l) tr->x[l] = (float*)take(MD4);
    for (int l = 0; l < depth; ++l) {
      TLayer& L = tr->L[l];
      L.x_mid = (float*)take(MD4);
      L.lse = (float*)take((size_t)B * m->Hq * ntok * 4);
      L.xn1 = (bf16_t*)take(MD2); L.q = (bf16_t*)take(MD2); L.k = (bf16_t*)take((size_t)M * kvD * 2);
      L.vt = (bf16_t*)take((size_t)B * m->Hkv * HEAD_DIM * tr->npad * 2);
      L.ao = (bf16_t*)take(MD2); L.y_attn = (bf16_t*)take(MD2); L.xn2 = (bf16_t*)take(MD2);
      L.h_pre = (bf16_t*)take((size_t)M * mlp * 2); L.h_post = (bf16_t*)take((size_t)M * mlp * 2);
      L.y_mlp = (bf16_t*)take(MD2);
      L.wqkvT = (bf16_t*)take((size_t)D * Nqkv * 2); L.woT = (bf16_t*)take((size_t)D * D * 2);
      L.w1T = (bf16_t*)take((size_t)D * mlp * 2); L.w2T = (bf16_t*)take((size_t)mlp * D * 2);
    }
    tr->a_patch = (bf16_t*)take((size_t)M * m->Kp * 2);
    tr->pe_pre = (bf16_t*)take((size_t)M * bott * 2); tr->pe_h = (bf16_t*)take((size_t)M * bott * 2);
    tr->xnf = (bf16_t*)take(MD2);
    tr->t_silu = (bf16_t*)take((size_t)B * D * 2);
    tr->pe_w2T = (bf16_t*)take((size_t)bott * D * 2); tr->wfinalT = (bf16_t*)take((size_t)D * m->Fout * 2);
    tr->e_sin = (float*)take((size_t)B * D * 4); tr->u1 = (float*)take((size_t)B * D * 4);
    tr->t_h = (float*)take((size_t)B * D * 4); tr->t_emb = (float*)take((size_t)B * D * 4);
    tr->mod = (float*)take((size_t)B * depth * 6 * D * 4);
    tr->pred = (float*)take((size_t)B * m->Cin * T * 4);
    tr->dx = (float*)take(MD4); tr->dpred = (float*)take((size_t)B * m->Cin * T * 4);
    tr->dmod = (float*)take((size_t)B * depth * 6 * D * 4);
    tr->part = (float*)take((size_t)B * train_nchunk(ntok) * 3 * D * 4);
    tr->red_part = (float*)take((size_t)train_red_blocks() * 4);
    tr->scal = (float*)take(64);
    tr->terms = (float*)take(64);
    tr->tw = (float2*)take((size_t)T * sizeof(float2));
    tr->ll_part = (float*)take((size_t)B * m->Cin * 8 * 4);
    tr->delta = (float*)take((size_t)B * m->Hq * ntok * 4);
    tr->dkv_part = (float*)take((size_t)B * m->Hq * ntok * 128 * 4);
    tr->dwqkv = (float*)take((size_t)Nqkv * D * 4);
    tr->dt_emb = (float*)take((size_t)B * D * 4);
    tr->du1 = (float*)take((size_t)B * D * 4);
    {
      const int Nall = depth * 6 * D;
      const size_t slabs = std::max((Nall + small_dx_slab(Nall) - 1) / small_dx_slab(Nall), (D + small_dx_slab(D) - 1) / small_dx_slab(D));
      tr->small_part = (float*)take(slabs * B * D * 4);
    }
    tr->dw_part = (float*)take((size_t)B * D * 4);
    size_t split_f = 0, colsum_f = 0;   // the largest scratch any weight gradient of the step asks for
    for (auto& sh : dw_shapes(m)) {
      const DwScratch need = jat_weight_grad_scratch(M, sh[0], sh[1], gemm_tn_ksplit(sh[0], sh[1], M), true);
      split_f = std::max(split_f, need.split_floats);
      colsum_f = std::max(colsum_f, need.colsum_floats);
    }
    tr->dw_split = (float*)take(split_f * 4);
    tr->zero_cell = take(256);
    tr->copy_jobs = (CopyJob*)take(n_f32 * sizeof(CopyJob));
    tr->dy = (bf16_t*)take(MD2); tr->dh = (bf16_t*)take((size_t)M * std::max(mlp, bott) * 2);
    tr->dxn = (bf16_t*)take(MD2); tr->dao = (bf16_t*)take(MD2); tr->dqkv = (bf16_t*)take((size_t)M * Nqkv * 2);
    tr->dy_m[0] = tr->dy_a[0] = tr->dy; tr->dy_m[1] = tr->dy_a[1] = tr->dy;   // one stream: every operand has one home
    tr->dh_b[0] = tr->dh_b[1] = tr->dh; tr->dq_b[0] = tr->dq_b[1] = tr->dqkv;
    if (tr->dw_async) {   // second home per operand (layer parity) + a separate one for the attention branch's dy: + ~0.4 GB at T = 1378
      tr->dy_m[1] = (bf16_t*)take(MD2); tr->dy_a[0] = (bf16_t*)take(MD2); tr->dy_a[1] = (bf16_t*)take(MD2);
      tr->dh_b[1] = (bf16_t*)take((size_t)M * std::max(mlp, bott) * 2);
      tr->dq_b[1] = (bf16_t*)take((size_t)M * Nqkv * 2);
    }
    tr->dyf = (bf16_t*)take((size_t)M * m->Fout * 2);
    tr->colsum_part = (float*)take(colsum_f * 4);
    if (pass == 0) {
      tr->blob_bytes = o;
      if (hipMalloc((void**)&tr->blob, o) != hipSuccess)
        return fail(JAT_E_HIP, "hipMalloc of %zu bytes for the training workspace failed", o);
      // zero once: the key padding of every V^T buffer must be 0 and is never written afterwards
      if (hipMemsetAsync(tr->blob, 0, o, s) != hipSuccess) return fail(JAT_E_HIP, "memset failed");
    }
  }
  {
    std::vector<CopyJob> jobs;   // the re-pack's fp32 copies: master slice -> the model's operand tensor
    for (const ParamDesc& e : m->params)
      if (e.form == F_F32 && m->has(e)) jobs.push_back(CopyJob{params_flat + tr->offset_of(e), m->at<float>(e), e.numel()});
    tr->n_copy_jobs = (int)jobs.size();
    if (hipMemcpyAsync(tr->copy_jobs, jobs.data(), jobs.size() * sizeof(CopyJob), hipMemcpyHostToDevice, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
      return fail(JAT_E_HIP, "copy-table upload failed");
  }
  const std::vector<float2> tw = make_twiddles(T);
  if (hipMemcpyAsync(tr->tw, tw.data(), tw.size() * sizeof(float2), hipMemcpyHostToDevice, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return fail(JAT_E_HIP, "twiddle upload failed");
  rc = build_transposes(tr, s);   // the model's own copies were packed from these very tensors by jat_model_load_weights
  if (rc != JAT_OK) return rc;
  if (hipStreamSynchronize(s) != hipSuccess) return fail(JAT_E_HIP, "trainer setup failed");
  *out = owner.release();
  return JAT_OK;
}

extern "C" int jat_trainer_set_grad_hook(jat_trainer* tr, void (*hook)(int64_t, int64_t, void*), void* user) {
  if (!tr) return fail(JAT_E_INVALID, "null argument");
  tr->hook = hook;
  tr->hook_user = user;
  return JAT_OK;
}

extern "C" int jat_trainer_set_regularisers(jat_trainer* tr, const float* dropout, const float* drop_path) {
  if (!tr || !dropout || !drop_path) return fail(JAT_E_INVALID, "null argument");
  for (int l = 0; l < tr->m->depth; ++l) {
    if (!(dropout[l] >= 0.f && dropout[l] < 1.f) || !(drop_path[l] >= 0.f && drop_path[l] < 1.f))
      return fail(JAT_E_INVALID, "layer %d: rates must be in [0, 1)", l);
    tr->p_drop[l] = dropout[l];
    tr->p_path[l] = drop_path[l];
  }
  return JAT_OK;
}

extern "C" int jat_trainer_set_latent_loss(jat_trainer* tr, double latent_weight, double freq_weight, double ms_weight,
                                           double consistency_weight, double low_freq_phase_ratio, double strict_cutoff,
                                           double soft_cutoff) {
  if (!tr) return fail(JAT_E_INVALID, "null argument");
  const LossSpec l{tr->loss.recon_eps, tr->loss.rw, latent_weight, freq_weight, ms_weight, consistency_weight,
                   low_freq_phase_ratio, strict_cutoff, soft_cutoff};
  JCHK(check_band_ratios(l));
  if (l.has_latent() && l.recon_eps > 0.0)
    return fail(JAT_E_STATE, "the latent perceptual loss is defined on top of the MSE loss only (train_ddp_v3mod2.py:889-896)");
  tr->loss = l;
  return JAT_OK;
}

extern "C" int jat_trainer_set_charbonnier(jat_trainer* tr, double eps) {
  if (!tr) return fail(JAT_E_INVALID, "null argument");
  if (!(eps >= 0.0)) return fail(JAT_E_INVALID, "eps must be >= 0 (0 selects the MSE loss)");
  if (eps > 0.0 && tr->loss.has_latent())
    return fail(JAT_E_STATE, "the latent perceptual loss is defined on top of the MSE loss only (train_ddp_v3mod2.py:889-896)");
  tr->loss.recon_eps = eps;
  return JAT_OK;
}

// The whole loss in one call (the v3mod3 trainer, train_ddp_v3mod3.py:400-434,955-969):
//   recon_weight * recon + latent_weight * (freq_weight * freq + ms_weight * ms + consistency_weight * cons)
// recon = Charbonnier(recon_eps) for recon_eps > 0, MSE for 0.  Everything is validated before anything is stored.
extern "C" int jat_trainer_set_loss_ex(jat_trainer* tr, double recon_eps, double recon_weight, double latent_weight,
                                       double freq_weight, double ms_weight, double consistency_weight,
                                       double low_freq_phase_ratio, double strict_cutoff, double soft_cutoff) {
  if (!tr) return fail(JAT_E_INVALID, "null argument");
  const LossSpec l{recon_eps, recon_weight, latent_weight, freq_weight, ms_weight, consistency_weight,
                   low_freq_phase_ratio, strict_cutoff, soft_cutoff};
  JCHK(check_recon_eps(l));
  JCHK(check_loss_weights(l));
  JCHK(check_band_ratios(l));
  tr->loss = l;
  return JAT_OK;
}

extern "C" int jat_trainer_loss_terms(jat_trainer* tr, float* out6, void* stream) {
  if (!tr || !out6) return fail(JAT_E_INVALID, "null argument");
  if (!tr->loss.has_latent()) return fail(JAT_E_STATE, "the latent perceptual loss is off (jat_trainer_set_latent_loss)");
  HIPCHK(hipMemcpyAsync(out6, tr->terms, 6 * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return JAT_OK;
}

extern "C" int jat_trainer_workspace_bytes(const jat_trainer* tr, size_t* out) {
  if (!tr || !out) return fail(JAT_E_INVALID, "null argument");
  *out = tr->blob_bytes;
  return JAT_OK;
}

extern "C" int jat_trainer_prepare(jat_trainer* tr, const float* hr_norm, float* cond, const float* noise,
                                   const float* cond_noise, float cond_noise_ratio, int32_t adaptive, const float* keep,
                                   const float* t, float* z_t, void* stream) {
  if (!tr || !hr_norm || !cond || !noise || !t || !z_t) return fail(JAT_E_INVALID, "null argument");
  hipStream_t s = (hipStream_t)stream;
  const int64_t per = (int64_t)tr->m->Cin * tr->T;
  if (cond_noise && cond_noise_ratio > 0.f && adaptive)   // lr_norm.std().clamp(0.5, 2.0)  (train_ddp_v3m2.py:553-556)
    KCHK(launch_tensor_std(cond, (int64_t)tr->B * tr->m->Cc * tr->T, tr->red_part, tr->scal + 8, tr->scal + 4, s));
  if ((cond_noise && cond_noise_ratio > 0.f) || keep)
    KCHK(launch_cond_augment(cond, cond_noise_ratio > 0.f ? cond_noise : nullptr, adaptive ? tr->scal + 4 : nullptr,
                             cond_noise_ratio, keep, tr->B, (int64_t)tr->m->Cc * tr->T, s));
  KCHK(launch_flow_mix(hr_norm, noise, t, z_t, tr->B, per, s));
  return JAT_OK;
}

extern "C" int jat_trainer_fwd_bwd(jat_trainer* tr, const float* z_t, const float* t, const float* x_cond,
                                   const float* target, const float* cond_clean, float loss_scale, uint64_t rng_seed,
                                   float* loss_out, float* x_pred_out, void* stream) {
  return jat_trainer_fwd_bwd_ex(tr, z_t, t, x_cond, target, cond_clean, loss_scale, rng_seed, loss_out, x_pred_out, 0, stream);
}

extern "C" int jat_trainer_fwd_bwd_ex(jat_trainer* tr, const float* z_t, const float* t, const float* x_cond,
                                      const float* target, const float* cond_clean, float loss_scale, uint64_t rng_seed,
                                      float* loss_out, float* x_pred_out, int32_t flags, void* stream) {
  if (!tr || !z_t || !t || !x_cond || !target) return fail(JAT_E_INVALID, "null argument");
  if (flags & ~(JAT_FB_ACCUMULATE | JAT_FB_NO_HOOK)) return fail(JAT_E_INVALID, "unknown flag bits 0x%x", (unsigned)flags);
  if (tr->loss.has_latent() && tr->loss.cw != 0.0 && !cond_clean)
    return fail(JAT_E_INVALID, "the consistency loss needs the clean condition latent (cond_clean)");
  if (!tr->m->loaded) return fail(JAT_E_STATE, "weights not loaded");
  hipStream_t s = (hipStream_t)stream;
  tr->seed = rng_seed;
  tr->accum = (flags & JAT_FB_ACCUMULATE) != 0;
  tr->no_hook = (flags & JAT_FB_NO_HOOK) != 0;
  JCHK(forward_train(tr, z_t, t, x_cond, s));
  JCHK(backward_train(tr, target, cond_clean, loss_scale, s));
  if (loss_out) HIPCHK(hipMemcpyAsync(loss_out, tr->scal, 4, hipMemcpyDeviceToDevice, s));
  if (x_pred_out)
    HIPCHK(hipMemcpyAsync(x_pred_out, tr->pred, (size_t)tr->B * tr->m->Cin * tr->T * 4, hipMemcpyDeviceToDevice, s));
  return JAT_OK;
}

extern "C" int jat_trainer_optim(jat_trainer* tr, float lr, float beta1, float beta2, float eps, float weight_decay,
                                 float max_grad_norm, float loss_scale, int32_t step, float* grad_norm_out, void* stream) {
  if (!tr) return fail(JAT_E_INVALID, "null argument");
  if (step < 1 || loss_scale <= 0.f) return fail(JAT_E_INVALID, "step must be >= 1 and loss_scale > 0");
  hipStream_t s = (hipStream_t)stream;
  KCHK(launch_grad_sqsum(tr->G, tr->total, tr->red_part, tr->scal + 2, s));
  KCHK(launch_adamw(tr->P, tr->G, tr->m1, tr->m2, tr->total, tr->scal + 2, 1.0f / loss_scale, max_grad_norm, lr, beta1, beta2,
                    eps, weight_decay, step, tr->ema, tr->ema_decay, s));
  if (grad_norm_out) HIPCHK(hipMemcpyAsync(grad_norm_out, tr->scal + 3, 4, hipMemcpyDeviceToDevice, s));
  return repack(tr, s);
}

extern "C" int jat_trainer_set_ema(jat_trainer* tr, float* ema_flat, float decay) {
  if (!tr) return fail(JAT_E_INVALID, "null argument");
  if (ema_flat) {
    if (!(decay >= 0.f && decay < 1.f)) return fail(JAT_E_INVALID, "ema decay must be in [0, 1)");
    if (((uintptr_t)ema_flat & 15u) != 0 || ema_flat == tr->P) return fail(JAT_E_INVALID, "ema_flat must be a 16-B aligned buffer of its own");
  }
  tr->ema = ema_flat;
  tr->ema_decay = ema_flat ? decay : 0.f;
  return JAT_OK;
}

extern "C" int jat_trainer_swap_ema(jat_trainer* tr, void* stream) {
  if (!tr) return fail(JAT_E_INVALID, "null argument");
  if (!tr->ema) return fail(JAT_E_STATE, "no moving average is set (jat_trainer_set_ema)");
  hipStream_t s = (hipStream_t)stream;
  KCHK(launch_swap_f32(tr->P, tr->ema, tr->total, s));
  return repack(tr, s);
}

// per-kernel entry point (unit parity, validation): reconstruction loss and d(loss * loss_scale)/d pred on n elements;
// eps > 0: Charbonnier (train_ddp_v3m2mod1.py:72-101), eps == 0: MSE (train_ddp_v3m2.py:585); work: 1024 + 2 floats
extern "C" int jat_k_recon_loss(const float* pred, const float* target, float* dpred, float* loss_out, int64_t n, double eps,
                                float loss_scale, void* work, size_t work_bytes, void* stream) {
  if (!pred || !target || !dpred || !loss_out || !work || n <= 0 || !(eps >= 0.0)) return fail(JAT_E_INVALID, "bad argument");
  const LossSpec l{eps};   // no latent term, weight 1
  const LossLaunch pl = plan_loss(l, n, 1);
  if (work_bytes < pl.recon_bytes) return fail(JAT_E_STATE, "work buffer too small: %zu < %zu bytes", work_bytes, pl.recon_bytes);
  hipStream_t s = (hipStream_t)stream;
  float *part = (float*)work, *loss2 = part + train_red_blocks();
  JCHK(run_loss(l, pl, pred, target, nullptr, nullptr, dpred, part, loss2, n, 1, loss_scale, s));
  HIPCHK(hipMemcpyAsync(loss_out, loss2, 4, hipMemcpyDeviceToDevice, s));
  return JAT_OK;
}

// which path launch_latent_loss takes at length T (csrc/train.hip plan_latent_loss); host only, launches nothing
extern "C" int jat_k_latent_loss_plan(int32_t T, int32_t* kind, int32_t* a, int32_t* b, int64_t* lds_bytes) {
  if (!kind || !a || !b || !lds_bytes || T <= 0) return fail(JAT_E_INVALID, "bad argument");
  const LatentLossPlan pl = plan_latent_loss(T);
  *kind = pl.kind; *a = pl.a; *b = pl.b; *lds_bytes = (int64_t)pl.lds;
  return JAT_OK;
}

// body of jat_k_latent_loss / jat_k_latent_loss_ex; `work` holds align_up(T*8, 256) + rows*32 bytes
static int k_latent_loss(const float* pred, const float* target, const float* lr, float* dpred, float* out6, int32_t rows, int32_t T,
                         const LossSpec& l, float loss_scale, void* work, size_t work_bytes, void* stream) {
  if (!pred || !target || !dpred || !out6 || !work || rows <= 0 || T <= 0) return fail(JAT_E_INVALID, "bad argument");
  // what launch_latent_loss would reject, before anything is copied or launched
  JCHK(check_band_ratios(l));
  LossLaunch pl = plan_loss(l, rows, T);
  pl.latent = true;   // this entry point IS the latent kernels: latent_weight == 0 leaves their reconstruction term
  if (pl.path.kind == 0)
    return fail(JAT_E_INVALID, "T %d is too long for the loss kernels: their LDS image needs %zu bytes", T, pl.path.lds);
  if (work_bytes < pl.latent_bytes) return fail(JAT_E_STATE, "work buffer too small: %zu < %zu bytes", work_bytes, pl.latent_bytes);
  hipStream_t s = (hipStream_t)stream;
  float2* tw = (float2*)work;
  float* part = (float*)((char*)work + pl.tw_bytes);
  const std::vector<float2> h = make_twiddles(T);
  HIPCHK(hipMemcpyAsync(tw, h.data(), h.size() * sizeof(float2), hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));
  return run_loss(l, pl, pred, target, lr, tw, dpred, part, out6, rows, T, loss_scale, s);
}

// per-kernel entry point (unit parity): the v3mod2 loss on [rows, T] tensors
extern "C" int jat_k_latent_loss(const float* pred, const float* target, const float* lr, float* dpred, float* out6,
                                 int32_t rows, int32_t T, double latent_weight, double freq_weight, double ms_weight,
                                 double consistency_weight, double low_freq_phase_ratio, double strict_cutoff,
                                 double soft_cutoff, float loss_scale, void* work, size_t work_bytes, void* stream) {
  const LossSpec l{0.0, 1.0, latent_weight, freq_weight, ms_weight, consistency_weight, low_freq_phase_ratio, strict_cutoff, soft_cutoff};
  return k_latent_loss(pred, target, lr, dpred, out6, rows, T, l, loss_scale, work, work_bytes, stream);
}

// the same with the v3mod3 reconstruction term (train_ddp_v3mod3.py:955-969): recon_weight * recon + latent_weight * (...), recon =
// Charbonnier(recon_eps) for recon_eps > 0, MSE for 0; out6[1] = the un-weighted recon term.  (0, 1) is jat_k_latent_loss, kernel
// for kernel.  Same work buffer and the same rejections before anything is launched.
extern "C" int jat_k_latent_loss_ex(const float* pred, const float* target, const float* lr, float* dpred, float* out6,
                                    int32_t rows, int32_t T, double recon_eps, double recon_weight, double latent_weight,
                                    double freq_weight, double ms_weight, double consistency_weight,
                                    double low_freq_phase_ratio, double strict_cutoff, double soft_cutoff, float loss_scale,
                                    void* work, size_t work_bytes, void* stream) {
  const LossSpec l{recon_eps, recon_weight, latent_weight, freq_weight, ms_weight, consistency_weight,
                   low_freq_phase_ratio, strict_cutoff, soft_cutoff};
  JCHK(check_recon_eps(l));
  JCHK(check_loss_weights(l));
  return k_latent_loss(pred, target, lr, dpred, out6, rows, T, l, loss_scale, work, work_bytes, stream);
}

// ---- per-kernel entry points of the training step (unit parity against fp64 references; include/jat_hip.h) ------------
// Each validates what its launcher would reject (JAT_E_INVALID, never a launch that fails), takes its scratch from the
// caller's `work` and calls the same launch_* the trainer calls.  Dropout sites are (seed, site, p) -> jat_drop_spec, as site().
namespace {
bool rate_ok(float p) { return p >= 0.f && p < 1.f; }
bool al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
}  // namespace

extern "C" int jat_k_attention_train(const uint16_t* q, const uint16_t* k, const uint16_t* vt, uint16_t* o, float* lse, int32_t B,
                                     int32_t N, int32_t Hq, int32_t Hkv, int32_t Npad, uint64_t seed, int32_t site, float p,
                                     void* stream) {
  if (!q || !k || !vt || !o || !lse) return fail(JAT_E_INVALID, "null argument");
  if (B <= 0 || N <= 0 || N > MAX_LEN || Hkv <= 0 || Hq <= 0 || Hq % Hkv != 0 || Npad % 64 != 0 || Npad < N)
    return fail(JAT_E_INVALID, "bad shape: B %d N %d (1..%d) Hq %d Hkv %d Npad %d", B, N, MAX_LEN, Hq, Hkv, Npad);
  if (site < 0 || !rate_ok(p)) return fail(JAT_E_INVALID, "site must be >= 0 and p in [0, 1)");
  AttnArgs a{};
  a.q = q; a.k = k; a.vt = vt; a.o = o; a.ldq = (int64_t)Hq * 64; a.ldk = (int64_t)Hkv * 64; a.ldo = (int64_t)Hq * 64;
  a.B = B; a.N = N; a.Hq = Hq; a.Hkv = Hkv; a.npad = Npad;
  a.scale_log2e = 0.125f * 1.4426950408889634f;
  a.lse = lse;
  a.drop = jat_drop_spec(seed, (uint32_t)site, p);
  KCHK(launch_attention(a, (hipStream_t)stream));
  return JAT_OK;
}

extern "C" int jat_k_attention_bwd(const uint16_t* q, const uint16_t* k, const uint16_t* vt, const uint16_t* o, const uint16_t* dout,
                                   const float* lse, uint16_t* dqkv, const float* rope_cos, const float* rope_sin, int32_t B,
                                   int32_t N, int32_t Hq, int32_t Hkv, int32_t Npad, uint64_t seed, int32_t site, float p,
                                   int32_t split_heads, void* work, size_t work_bytes, void* stream) {
  if (!q || !k || !vt || !o || !dout || !lse || !dqkv || !rope_cos || !rope_sin || !work) return fail(JAT_E_INVALID, "null argument");
  if (B <= 0 || N <= 0 || N > MAX_LEN || Hkv <= 0 || Hq <= 0 || Hq % Hkv != 0 || Npad % 64 != 0 || Npad < N)
    return fail(JAT_E_INVALID, "bad shape: B %d N %d (1..%d) Hq %d Hkv %d Npad %d", B, N, MAX_LEN, Hq, Hkv, Npad);
  if (site < 0 || !rate_ok(p)) return fail(JAT_E_INVALID, "site must be >= 0 and p in [0, 1)");
  const size_t rows = (size_t)B * Hq * N, delta_b = align_up(rows * 4, 256);
  const size_t need = delta_b + (split_heads ? rows * 128 * 4 : 0);
  if (work_bytes < need) return fail(JAT_E_INVALID, "work needs %zu bytes", need);
  float* delta = (float*)work;
  float* dkv_part = split_heads ? (float*)((char*)work + delta_b) : nullptr;
  KCHK(launch_attention_bwd(q, k, vt, o, dout, lse, delta, dqkv, rope_cos, rope_sin, B, N, Hq, Hkv, Npad,
                            jat_drop_spec(seed, (uint32_t)site, p), dkv_part, (hipStream_t)stream));
  return JAT_OK;
}

extern "C" int jat_k_norm_bwd(const float* x, const uint16_t* dy, const float* w, const float* scale, int64_t mod_bstride,
                              float* dx, int32_t accumulate, float* dshift, float* dscale, int64_t dmod_bstride, float* dw,
                              int32_t B, int32_t D, int32_t ntok, int32_t mode, void* work, size_t work_bytes, void* stream) {
  if (!x || !dy || !dx || !work) return fail(JAT_E_INVALID, "null argument");
  if (D % 256 != 0 || D <= 0 || D > 2048) return fail(JAT_E_INVALID, "D = %d: a multiple of 256 up to 2048", D);
  if (B <= 0 || ntok <= 0) return fail(JAT_E_INVALID, "B and ntok must be positive");
  if (mode != JAT_NORM_RMS_W && mode != JAT_NORM_LN_NOAFFINE) return fail(JAT_E_INVALID, "mode must be 0 (RMS) or 1 (LayerNorm)");
  if (mode == JAT_NORM_LN_NOAFFINE && (w || dw)) return fail(JAT_E_INVALID, "the LayerNorm (mode 1) has no weight");
  if (scale && (mod_bstride < 0 || mod_bstride % 4 != 0 || !al16(scale)))
    return fail(JAT_E_INVALID, "scale rows must be 16-byte aligned (mod_bstride %% 4 == 0)");
  if ((dshift || dscale) && dmod_bstride < D) return fail(JAT_E_INVALID, "dmod_bstride must be >= D");
  if (!al16(x) || !al16(dx) || !al16(dy) || (w && !al16(w))) return fail(JAT_E_INVALID, "x, dy, dx and w must be 16-byte aligned");
  const size_t part_f = (size_t)B * train_nchunk(ntok) * 3 * D, need = (part_f + (size_t)B * D) * 4;
  if (work_bytes < need) return fail(JAT_E_INVALID, "work needs %zu bytes", need);
  float* part = (float*)work;
  KCHK(launch_norm_bwd(x, dy, w, scale, mod_bstride, dx, accumulate ? 1 : 0, part, part + part_f, dshift, dscale, dmod_bstride,
                       dw, 0, B, D, ntok, mode, (hipStream_t)stream));
  return JAT_OK;
}

extern "C" int jat_k_gate_bwd(const float* dx, const uint16_t* y, const float* gate, int64_t gate_bstride, uint16_t* dy,
                              float* dgate, int64_t dgate_bstride, int32_t B, int32_t D, int32_t ntok, uint64_t seed,
                              int32_t path_site, float path_p, int32_t elem_site, float elem_p, void* work, size_t work_bytes,
                              void* stream) {
  if (!dx || !y || !gate || !dy || !dgate || !work) return fail(JAT_E_INVALID, "null argument");
  if (B <= 0 || ntok <= 0 || D <= 0 || D % 4 != 0) return fail(JAT_E_INVALID, "B, ntok > 0 and D a positive multiple of 4");
  if (gate_bstride < 0 || gate_bstride % 4 != 0 || dgate_bstride < D) return fail(JAT_E_INVALID, "bad gate strides");
  if (!al16(dx) || !al16(gate) || ((uintptr_t)y & 7u) || ((uintptr_t)dy & 7u)) return fail(JAT_E_INVALID, "misaligned operand");
  if (path_site < 0 || elem_site < 0 || !rate_ok(path_p) || !rate_ok(elem_p)) return fail(JAT_E_INVALID, "bad dropout site");
  const size_t need = (size_t)B * train_nchunk(ntok) * D * 4;
  if (work_bytes < need) return fail(JAT_E_INVALID, "work needs %zu bytes", need);
  KCHK(launch_gate_bwd(dx, y, gate, gate_bstride, dy, (float*)work, dgate, dgate_bstride, B, D, ntok,
                       jat_drop_spec(seed, (uint32_t)path_site, path_p), jat_drop_spec(seed, (uint32_t)elem_site, elem_p),
                       (hipStream_t)stream));
  return JAT_OK;
}

extern "C" int jat_k_resid_gate(const float* x_in, const uint16_t* y, const float* gate, int64_t gate_bstride, float* x_out,
                                int32_t M, int32_t D, int32_t ntok, uint64_t seed, int32_t path_site, float path_p,
                                int32_t elem_site, float elem_p, void* stream) {
  if (!x_in || !y || !gate || !x_out) return fail(JAT_E_INVALID, "null argument");
  if (M <= 0 || ntok <= 0 || D <= 0 || D % 8 != 0) return fail(JAT_E_INVALID, "M, ntok > 0 and D a positive multiple of 8");
  if (gate_bstride < 0 || gate_bstride % 4 != 0) return fail(JAT_E_INVALID, "gate_bstride must be a multiple of 4");
  if (!al16(x_in) || !al16(x_out) || !al16(gate) || !al16(y)) return fail(JAT_E_INVALID, "misaligned operand");
  if (path_site < 0 || elem_site < 0 || !rate_ok(path_p) || !rate_ok(elem_p)) return fail(JAT_E_INVALID, "bad dropout site");
  KCHK(launch_resid_gate(x_in, y, gate, gate_bstride, x_out, M, D, ntok, jat_drop_spec(seed, (uint32_t)path_site, path_p),
                         jat_drop_spec(seed, (uint32_t)elem_site, elem_p), (hipStream_t)stream));
  return JAT_OK;
}

extern "C" int jat_k_gelu(const uint16_t* in, uint16_t* out, int64_t n, uint64_t seed, int32_t site, float p, void* stream) {
  if (!in || !out) return fail(JAT_E_INVALID, "null argument");
  if (n <= 0 || n % 8 != 0 || !al16(in) || !al16(out)) return fail(JAT_E_INVALID, "n must be a positive multiple of 8, 16-B aligned");
  if (site < 0 || !rate_ok(p)) return fail(JAT_E_INVALID, "site must be >= 0 and p in [0, 1)");
  KCHK(launch_gelu_bf16(in, out, n, jat_drop_spec(seed, (uint32_t)site, p), (hipStream_t)stream));
  return JAT_OK;
}

extern "C" int jat_k_gelu_bwd(const uint16_t* pre, uint16_t* d, int64_t n, uint64_t seed, int32_t site, float p, void* stream) {
  if (!pre || !d) return fail(JAT_E_INVALID, "null argument");
  if (n <= 0 || n % 8 != 0 || !al16(pre) || !al16(d)) return fail(JAT_E_INVALID, "n must be a positive multiple of 8, 16-B aligned");
  if (site < 0 || !rate_ok(p)) return fail(JAT_E_INVALID, "site must be >= 0 and p in [0, 1)");
  KCHK(launch_gelu_bwd(pre, d, n, jat_drop_spec(seed, (uint32_t)site, p), (hipStream_t)stream));
  return JAT_OK;
}

extern "C" int jat_k_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                           float weight_decay, float max_grad_norm, float loss_scale, int32_t step, float* grad_norm_out,
                           void* work, size_t work_bytes, void* stream) {
  if (!p || !g || !m || !v || !work) return fail(JAT_E_INVALID, "null argument");
  if (n <= 0 || n % 4 != 0 || !al16(p) || !al16(g) || !al16(m) || !al16(v))
    return fail(JAT_E_INVALID, "n must be a positive multiple of 4, buffers 16-B aligned");
  if (step < 1 || !(loss_scale > 0.f)) return fail(JAT_E_INVALID, "step must be >= 1 and loss_scale > 0");
  const size_t need = ((size_t)train_red_blocks() + 2) * 4;
  if (work_bytes < need) return fail(JAT_E_INVALID, "work needs %zu bytes", need);
  hipStream_t s = (hipStream_t)stream;
  float* part = (float*)work;
  float* norm2 = part + train_red_blocks();
  // as jat_trainer_optim chains them: sum of squares of the scaled gradients, then clip + AdamW
  KCHK(launch_grad_sqsum(g, n, part, norm2, s));
  KCHK(launch_adamw(p, (float*)g, m, v, n, norm2, 1.0f / loss_scale, max_grad_norm, lr, beta1, beta2, eps, weight_decay, step,
                    nullptr, 0.f, s));
  if (grad_norm_out) HIPCHK(hipMemcpyAsync(grad_norm_out, norm2 + 1, 4, hipMemcpyDeviceToDevice, s));
  return JAT_OK;
}

extern "C" int jat_k_adamw_ema(float* p, const float* g, float* m, float* v, float* ema, int64_t n, float lr, float beta1,
                               float beta2, float eps, float weight_decay, float max_grad_norm, float loss_scale, float ema_decay,
                               int32_t step, float* grad_norm_out, void* work, size_t work_bytes, void* stream) {
  if (!p || !g || !m || !v || !ema || !work) return fail(JAT_E_INVALID, "null argument");
  if (n <= 0 || n % 4 != 0 || !al16(p) || !al16(g) || !al16(m) || !al16(v) || !al16(ema))
    return fail(JAT_E_INVALID, "n must be a positive multiple of 4, buffers 16-B aligned");
  if (step < 1 || !(loss_scale > 0.f)) return fail(JAT_E_INVALID, "step must be >= 1 and loss_scale > 0");
  if (!(ema_decay >= 0.f && ema_decay < 1.f)) return fail(JAT_E_INVALID, "ema decay must be in [0, 1)");
  if (ema == p || ema == m || ema == v || ema == g) return fail(JAT_E_INVALID, "ema must be a buffer of its own");
  const size_t need = ((size_t)train_red_blocks() + 2) * 4;
  if (work_bytes < need) return fail(JAT_E_INVALID, "work needs %zu bytes", need);
  hipStream_t s = (hipStream_t)stream;
  float* part = (float*)work;
  float* norm2 = part + train_red_blocks();
  KCHK(launch_grad_sqsum(g, n, part, norm2, s));
  KCHK(launch_adamw(p, (float*)g, m, v, n, norm2, 1.0f / loss_scale, max_grad_norm, lr, beta1, beta2, eps, weight_decay, step, ema,
                    ema_decay, s));
  if (grad_norm_out) HIPCHK(hipMemcpyAsync(grad_norm_out, norm2 + 1, 4, hipMemcpyDeviceToDevice, s));
  return JAT_OK;
}

// the weight / bias gradient of one Linear, as the trainer's weight_grad runs it; ksplit == 0: the trainer's own choice.
// work: 256 zero-cell bytes, then the split slices, then the column-sum partials
extern "C" int jat_k_weight_grad(const uint16_t* dY, const uint16_t* X, float* dW, float* db, int32_t tokens, int32_t out,
                                 int32_t in, int32_t ksplit, void* work, size_t work_bytes, void* stream) {
  return jat_k_weight_grad_ex(dY, X, dW, db, tokens, out, in, ksplit, work, work_bytes, 0, stream);
}
extern "C" int jat_k_weight_grad_ex(const uint16_t* dY, const uint16_t* X, float* dW, float* db, int32_t tokens, int32_t out,
                                    int32_t in, int32_t ksplit, void* work, size_t work_bytes, int32_t accumulate, void* stream) {
  if (!gemm_tn_supports(out, in)) return fail(JAT_E_INVALID, "out and in must be multiples of 128");
  if (tokens <= 0) return fail(JAT_E_INVALID, "tokens must be positive");
  if (ksplit == 0) ksplit = gemm_tn_ksplit(out, in, tokens);
  if (ksplit < 1 || ksplit > (tokens + 63) / 64) return fail(JAT_E_INVALID, "bad ksplit");
  const DwScratch sc = jat_weight_grad_scratch(tokens, out, in, ksplit, db != nullptr);
  const size_t need = 256 + (sc.split_floats + sc.colsum_floats) * 4;
  if (!work || work_bytes < need) return fail(JAT_E_INVALID, "work needs %zu bytes", need);
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipMemsetAsync(work, 0, 256, s));   // the zero cell ragged token tiles are padded from
  float* split = (float*)((char*)work + 256);
  return jat_weight_grad(dY, X, dW, db, tokens, out, in, ksplit, work, split, split + sc.split_floats, accumulate != 0, s);
}

// which launch a weight gradient [out, in] over `tokens` rows is (gemm_tn.hip): the output tile (128 or 256) and the K slices;
// host only, launches nothing
extern "C" int jat_k_weight_grad_plan(int32_t out, int32_t in, int32_t tokens, int32_t* tile, int32_t* ksplit) {
  if (!tile || !ksplit || out <= 0 || in <= 0 || tokens <= 0) return fail(JAT_E_INVALID, "bad argument");
  if (!gemm_tn_supports(out, in)) return fail(JAT_E_INVALID, "out and in must be multiples of 128");
  *tile = gemm_tn_tile(out, in);
  *ksplit = gemm_tn_ksplit(out, in, tokens);
  return JAT_OK;
}

extern "C" int jat_k_small_dw(const float* dy, int64_t ldy, const float* x, int64_t ldx, float* dW, float* db, int32_t B, int32_t N,
                              int32_t K, int32_t silu_x, void* stream) {
  if (!dy || !x || !dW) return fail(JAT_E_INVALID, "null argument");
  if (B <= 0 || B > 64) return fail(JAT_E_INVALID, "B = %d: 1..64 rows", B);
  if (N <= 0 || K <= 0 || K % 4 != 0 || ldy < N || ldx < K || ldx % 4 != 0)
    return fail(JAT_E_INVALID, "N > 0, K a positive multiple of 4, ldy >= N, ldx >= K a multiple of 4");
  if (!al16(x) || !al16(dW)) return fail(JAT_E_INVALID, "x and dW must be 16-byte aligned");
  KCHK(launch_small_dw(dy, ldy, x, ldx, dW, db, B, N, K, silu_x ? 1 : 0, 0, (hipStream_t)stream));
  return JAT_OK;
}

extern "C" int jat_k_small_dx(const float* dy, int64_t ldy, const void* W, int32_t w_is_bf16, float* dx, int32_t B, int32_t N,
                              int32_t K, int32_t accumulate, const float* silu_pre, void* work, size_t work_bytes, void* stream) {
  if (!dy || !W || !dx || !work) return fail(JAT_E_INVALID, "null argument");
  if (B <= 0 || B > 32) return fail(JAT_E_INVALID, "B = %d: 1..32 rows", B);
  if (N <= 0 || K <= 0 || K % 4 != 0 || ldy < N) return fail(JAT_E_INVALID, "N > 0, K a positive multiple of 4, ldy >= N");
  if (((uintptr_t)W & (w_is_bf16 ? 7u : 15u)) || !al16(work)) return fail(JAT_E_INVALID, "misaligned W or work");
  const int slab = small_dx_slab(N);
  const size_t need = (size_t)((N + slab - 1) / slab) * B * K * 4;
  if (work_bytes < need) return fail(JAT_E_INVALID, "work needs %zu bytes", need);
  KCHK(launch_small_dx(dy, ldy, W, w_is_bf16 ? 1 : 0, (float*)work, dx, B, N, K, accumulate ? 1 : 0, silu_pre, (hipStream_t)stream));
  return JAT_OK;
}

// Re-derive every operand copy (bf16 weights, transposed copies, fp32 operand tensors) from the flat master buffer,
// e.g. after the caller overwrote parameters (checkpoint resume, train_ddp_v3m2.py:443-500).
extern "C" int jat_trainer_repack(jat_trainer* tr, void* stream) {
  if (!tr) return fail(JAT_E_INVALID, "null argument");
  return repack(tr, (hipStream_t)stream);
}
