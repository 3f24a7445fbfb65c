// The model's parameters and the layout of its packed allocation, each written once (jat_internal.h: ParamDesc, BlobSlot).
// Both depend on the configuration alone.  Names and shapes: reference src/models/jat_audiosr_v3.py:350-386.
#include "jat_internal.h"

void jat_describe_params(jat_model* m) {
  const int D = m->D, kvD = m->kvD, mlp = m->mlp, bott = m->bott, depth = m->depth, Kp = m->Kp, Fout = m->Fout;
  const bool keep32 = m->cfg.norm_mode == JAT_NORM_RMS_W;   // fp32 fold sources of the sampler (RMSNorm models only)
  const bool group5 = m->Hq / m->Hkv == 5;                  // group-major QKV copy of the fused QKV+attention kernel
  m->layers.resize(depth);   // never resized again: m->slots points into it

  // ---- layout: every tensor of the blob in order, 256-byte aligned; returns the tensor's byte offset ----
  size_t off = 0;
  auto bump = [&](size_t bytes) { const size_t o = off; off += align_up(bytes, 256); return o; };
  auto half = [&](bf16_t*& p, size_t n) { const size_t o = bump(n * 2); m->slots.push_back({o, &p, nullptr}); return o; };
  auto full = [&](float*& p, size_t n) { const size_t o = bump(n * 4); m->slots.push_back({o, nullptr, &p}); return o; };
  const size_t o_pe_w1 = half(m->pe_w1, (size_t)bott * Kp), o_pe_w2 = half(m->pe_w2, (size_t)D * bott);
  const size_t o_wada = half(m->wada, (size_t)depth * 6 * D * D), o_wfinal = half(m->wfinal, (size_t)Fout * D);
  struct BlockOff { size_t qkv, wo, w1, w2, n1, n2, b1, b2; };
  std::vector<BlockOff> ob(depth);
  for (int l = 0; l < depth; ++l) {
    LayerW& L = m->layers[l];
    ob[l].qkv = half(L.wqkv, (size_t)(D + 2 * kvD) * D); ob[l].wo = half(L.wo, (size_t)D * D);
    if (group5) half(L.wqkv_g, (size_t)(D + 2 * kvD) * D);
    ob[l].w1 = half(L.w1, (size_t)mlp * D); ob[l].w2 = half(L.w2, (size_t)D * mlp);
    ob[l].n1 = full(L.norm1, D); ob[l].n2 = full(L.norm2, D);
    ob[l].b1 = full(L.b1, mlp); ob[l].b2 = full(L.b2, D);
    if (keep32) {
      full(L.q32, (size_t)D * D); full(L.k32, (size_t)kvD * D); full(L.v32, (size_t)kvD * D);
      full(L.w132, (size_t)mlp * D);
    }
  }
  if (keep32) full(m->wfinal32, (size_t)Fout * D);
  const size_t o_pe_b1 = full(m->pe_b1, bott), o_pe_b2 = full(m->pe_b2, D);
  const size_t o_te_w1 = full(m->te_w1, (size_t)D * D), o_te_b1 = full(m->te_b1, D);
  const size_t o_te_w2 = full(m->te_w2, (size_t)D * D), o_te_b2 = full(m->te_b2, D);
  const size_t o_bada = full(m->bada, (size_t)depth * 6 * D), o_fn = full(m->final_norm, D), o_bfinal = full(m->bfinal, Fout);
  full(m->rope_cos, (size_t)MAX_LEN * 32); full(m->rope_sin, (size_t)MAX_LEN * 32); full(m->rope_invf, 32);
  m->blob_bytes = off;

  // ---- the parameters: head, blocks, final layer ----
  int block = -1;
  std::string prefix;
  auto add = [&](int id, const char* name, int rows, int cols, ParamForm form, size_t dst, bool rms_only = false) {
    m->params.push_back(ParamDesc{id, block, prefix + name, rows, cols, form, dst, rms_only});
  };
  add(P_PE_W1, "patch_embed.proj.0.weight", bott, Kp, F_BF16, o_pe_w1);
  add(P_PE_B1, "patch_embed.proj.0.bias", bott, 1, F_F32, o_pe_b1);
  add(P_PE_W2, "patch_embed.proj.2.weight", D, bott, F_BF16, o_pe_w2);
  add(P_PE_B2, "patch_embed.proj.2.bias", D, 1, F_F32, o_pe_b2);
  add(P_TE_W1, "t_embedder.1.weight", D, D, F_F32, o_te_w1);
  add(P_TE_B1, "t_embedder.1.bias", D, 1, F_F32, o_te_b1);
  add(P_TE_W2, "t_embedder.3.weight", D, D, F_F32, o_te_w2);
  add(P_TE_B2, "t_embedder.3.bias", D, 1, F_F32, o_te_b2);
  for (block = 0; block < depth; ++block) {
    const BlockOff& o = ob[block];
    prefix = "blocks." + std::to_string(block) + ".";
    add(P_N1, "norm1.weight", D, 1, F_F32, o.n1, true);
    add(P_N2, "norm2.weight", D, 1, F_F32, o.n2, true);
    add(P_Q, "attn.q_proj.weight", D, D, F_BF16_ROPE, o.qkv);                                // fused [Wq; Wk; Wv]
    add(P_K, "attn.k_proj.weight", kvD, D, F_BF16_ROPE, o.qkv + (size_t)D * D * 2);
    add(P_V, "attn.v_proj.weight", kvD, D, F_BF16, o.qkv + (size_t)(D + kvD) * D * 2);
    add(P_O, "attn.out_proj.weight", D, D, F_BF16, o.wo);
    add(P_W1, "mlp.0.weight", mlp, D, F_BF16, o.w1);
    add(P_B1, "mlp.0.bias", mlp, 1, F_F32, o.b1);
    add(P_W2, "mlp.3.weight", D, mlp, F_BF16, o.w2);
    add(P_B2, "mlp.3.bias", D, 1, F_F32, o.b2);
    add(P_ADA_W, "adaLN_modulation.1.weight", 6 * D, D, F_BF16, o_wada + (size_t)block * 6 * D * D * 2);
    add(P_ADA_B, "adaLN_modulation.1.bias", 6 * D, 1, F_F32, o_bada + (size_t)block * 6 * D * 4);
  }
  prefix.clear();   // block == depth: the final layer
  add(P_FN, "final_layer.0.weight", D, 1, F_F32, o_fn, true);
  add(P_WF, "final_layer.1.weight", Fout, D, F_BF16, o_wfinal);
  add(P_BF, "final_layer.1.bias", Fout, 1, F_F32, o_bfinal);
}
