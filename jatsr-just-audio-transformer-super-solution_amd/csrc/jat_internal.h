// Internals shared by the C-ABI translation units (jat_api.cpp: model / forward / sampler; jat_train.cpp: training step).
#pragma once
#include "../../include/jat_hip.h"

#include <hip/hip_runtime.h>

#include <map>
#include <memory>
#include <string>
#include <vector>

#include "jat_kernels.h"

int jat_fail(int code, const char* fmt, ...);
#define fail jat_fail
#define HIPCHK(expr)                                                                                   \
  do {                                                                                                 \
    hipError_t e__ = (expr);                                                                           \
    if (e__ != hipSuccess) return fail(JAT_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), \
                                       __FILE__, __LINE__);                                            \
  } while (0)
#define JCHK(expr)            \
  do {                        \
    int r__ = (expr);         \
    if (r__ != JAT_OK) return r__; \
  } while (0)
#define KCHK(expr)                                                                            \
  do {                                                                                        \
    hipError_t e__ = (expr);                                                                  \
    if (e__ != hipSuccess) return fail(JAT_E_HIP, "%s: %s", #expr, hipGetErrorString(e__));   \
  } while (0)

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
static constexpr int MAX_LEN = 2048;  // jat_audiosr_v3.py:361
static constexpr int HEAD_DIM = 64;

// One model parameter, described once (jat_params.cpp): its name in the reference's state_dict, its size, the form the kernels
// read it in, where that operand copy lives in the packed allocation, the block it belongs to.  The loader, the trainer's table
// validation and the trainer's re-pack all walk jat_model::params.
enum ParamId {
  P_PE_W1, P_PE_B1, P_PE_W2, P_PE_B2, P_TE_W1, P_TE_B1, P_TE_W2, P_TE_B2,                   // head: patch embed, t_embedder
  P_N1, P_N2, P_Q, P_K, P_V, P_O, P_W1, P_B1, P_W2, P_B2, P_ADA_W, P_ADA_B,                 // one of each per block
  P_FN, P_WF, P_BF,                                                                         // final layer
  P_COUNT
};
enum ParamForm { F_F32, F_BF16, F_BF16_ROPE };   // fp32 copy, operand-dtype cast, cast with q/k rows pair-interleaved per head (RoPE pairs share a lane)
struct ParamDesc {
  int id;             // ParamId
  int block;          // -1: head, 0 .. depth-1: that block, depth: final layer
  std::string name;
  int rows, cols;     // numel = rows * cols (a vector: cols == 1)
  ParamForm form;
  size_t dst;         // byte offset of the operand copy in jat_model::blob (a slice of a shared tensor: K and V inside wqkv,
                      // block l's rows of wada / bada)
  bool rms_only;      // a norm weight: no source tensor in a LayerNorm model, whose copy is constant ones
  int64_t numel() const { return (int64_t)rows * cols; }
};
// a pointer of jat_model / LayerW into the packed allocation: *field = blob + off once the blob exists
struct BlobSlot {
  size_t off;
  bf16_t** h;
  float** f;
};

struct LayerW {
  bf16_t *wqkv, *wo, *w1, *w2;  // [D+2kvD, D], [D, D], [mlp, D], [D, mlp]
  bf16_t* wqkv_g = nullptr;     // group-major copy [Hkv][5*64 + 64 + 64][D] for the fused QKV+attention kernel (Hq/Hkv == 5)
  float *norm1, *norm2, *b1, *b2;
  float *q32 = nullptr, *k32 = nullptr, *v32 = nullptr, *w132 = nullptr;   // fp32 copies: sources of the sampler's folded weights
};

// Per-step folded weights of the sampler (RMSNorm models): W' = W diag(w_norm (1 + scale)) and shift @ W^T for every
// (step, layer) of a fixed schedule — input independent, built once per (model weights, steps) and shared by every sampler
// bucket (B, T) with that step count.  ~25 GB for v3mod2 at 50 steps: HBM capacity (288 GB) spent to delete the two norm
// kernels of every block from the captured graph.
struct FoldTable {
  int steps = 0;
  bf16_t *qkv_g = nullptr, *qkv_i = nullptr;   // [steps][depth][D+2kvD][D]: group-major (fused QKV+attention) / pair-interleaved
  bf16_t *w1 = nullptr, *wfinal = nullptr;     // [steps][depth][mlp][D], [Fout][D]
  float *bq_g = nullptr, *bq_i = nullptr, *bf = nullptr;   // [steps][depth][D+2kvD] x2, [steps][depth][mlp]
  std::vector<void*> allocs;
  ~FoldTable() { for (void* p : allocs) (void)hipFree(p); }
};

// Behaviour switches of one model handle: defaults from the JAT_* environment variables, read ONCE in jat_model_create (nothing on the
// per-call enqueue path touches the environment), changed per handle with jat_model_set_switch.
struct jat_switches {
  int fuse_qkv_attn = 1;   // JAT_FUSE_QKV_ATTN: 0 separate QKV GEMM + attention, 1 fused when B * Hkv blocks fill the chip, 2 always (128 tokens)
  int qkv_split = 1;       // JAT_QKV_SPLIT:     K-slices for the QKV GEMM of small buckets
  int fuse_finish = 1;     // JAT_FUSE_FINISH:   split-K finishing pass fused with the norm that follows it
  int fold_norm = 1;       // JAT_FOLD_NORM:     sampler norm folding (0 off, 1 buckets above kSplitMaxRows, 2 every bucket)
  int split_patch = 1;     // JAT_SPLIT_PATCH:   CFG sampler: condition half of the first patch-embed Linear computed once per run
  int fold_cap_mb = 0;     // JAT_FOLD_CAP_MB:   upper bound on the folded-weight table (0 = none); beyond it the sampler keeps the norm kernels
  int patch_split = 1;     // JAT_PATCH_SPLIT:   first patch-embed Linear as K slices + bias/GELU finishing pass when its tiles leave CU slots empty
  int fuse_euler = 1;      // JAT_FUSE_EULER:    CFG sampler: CFG combine + Euler step in the final Linear's epilogue, latent kept in patch layout
};
// measurement aid (bench.py roofline leg): HIP-event brackets around the launches of one GEMM call site of THIS model
struct GemmProf {
  int site = -1, n = 0, variant = -1;
  double flops = 0.0;
  hipStream_t stream = nullptr;
  std::vector<hipEvent_t> ev;
};

struct jat_model {
  jat_config cfg;
  jat_switches sw;
  mutable GemmProf prof;
  int D, depth, Hq, Hkv, kvD, mlp, bott, Cin, Cc, P, Kp, Fout;
  bool loaded = false;
  char* blob = nullptr;  // one device allocation holding every packed tensor (allocated by the first load)
  size_t blob_bytes = 0;
  std::vector<ParamDesc> params;   // head, blocks 0 .. depth-1, final layer; built with the blob's layout by jat_describe_params
  std::vector<BlobSlot> slots;
  bool has(const ParamDesc& e) const { return !e.rms_only || cfg.norm_mode == JAT_NORM_RMS_W; }
  template <class T> T* at(const ParamDesc& e) const { return (T*)(blob + e.dst); }
  bf16_t *pe_w1, *pe_w2, *wada, *wfinal;
  float *pe_b1, *pe_b2, *te_w1, *te_b1, *te_w2, *te_b2, *bada, *final_norm, *bfinal, *rope_cos, *rope_sin, *rope_invf;
  std::vector<LayerW> layers;
  // GEMM tile/pipeline variant per call site: qkv, out_proj, fc1, fc2, everything else (gemm_variants.h)
  int variants[5] = {-1, -1, -1, -1, -1};  // -1: choose by shape (gemm_plan.h)
  mutable int last_fold_np = 0;            // partial-sum slots per row written by the latest folding producer
  float* wfinal32 = nullptr;               // fp32 copy of the final Linear's weight (fold source)
  bool fold_src_ok = false;                // fp32 copies match the packed weights (false after a training re-pack)
  std::map<std::vector<uint32_t>, std::shared_ptr<FoldTable>> fold_cache;   // by the list of distinct evaluation times (fp32 bits); dropped whenever the weights change
  bool group_copy_stale = false;           // the training re-pack skips wqkv_g: the fused QKV+attention kernel is off until
                                           // the next full jat_model_load_weights
};
enum { G_QKV = 0, G_OUT = 1, G_FC1 = 2, G_FC2 = 3, G_OTHER = 4 };

// C[M,N] = A[M,K] W[N,K]^T through the planner (gemm_plan.h; plan == nullptr: a plain GEMM of the call site) and the profiling
// bracket of jat_api.cpp
struct GemmPlan;
int jat_gemm(const jat_model* m, int site, const bf16_t* A, int64_t lda, const bf16_t* W, int64_t ldw, int M, int N, int K,
             int epi, GemmArgs extra, hipStream_t s, const GemmPlan* plan = nullptr);
// jat_params.cpp: lay out the packed allocation (m->blob_bytes, m->slots) and describe every parameter (m->params) from the
// configuration alone; allocates and launches nothing.  Called once, by jat_model_create.
void jat_describe_params(jat_model* m);
// Full load (jat_model_load_weights): every parameter of m->params looked up by name, checked and converted to its operand
// copy, then the derived copies (group-major QKV, fold sources, constant-ones norm weights, RoPE tables); synchronises `s`.
// The trainer's re-pack after an optimiser step is jat_train.cpp's repack(), which walks the same table.
int jat_pack_weights(jat_model* m, const jat_tensor_ref* named, int32_t n, hipStream_t s);

// One weight gradient dW[out,in] = dY^T X (+ db[out] = column sums of dY when db) from token-major dY [tokens,out], X [tokens,in]
// (gemm_tn.hip): the GEMM, the ordered sum of its K slices when ksplit > 1, the column sum.  acc: added into dW / db, in the GEMM's
// epilogue when there is one slice, in the sum of the slices otherwise.  zeros: >= 16 zero bytes; split / colsum: scratch of
// jat_weight_grad_scratch(...) floats.  Both the trainer and jat_k_weight_grad_ex run this.
struct DwScratch { size_t split_floats, colsum_floats; };
DwScratch jat_weight_grad_scratch(int tokens, int out, int in, int ksplit, bool with_db);
int jat_weight_grad(const bf16_t* dY, const bf16_t* X, float* dW, float* db, int tokens, int out, int in, int ksplit,
                    const void* zeros, float* split, float* colsum, bool acc, hipStream_t s);

// ---- the training loss (jat_loss.cpp): rw * recon + lw * (fw * freq + mw * ms + cw * cons), recon = Charbonnier(recon_eps) for
// recon_eps > 0, MSE for 0.  Defaults: the V3 trainer's plain MSE.  A new loss variant is a field here and a branch in run_loss.
struct LossSpec {
  double recon_eps = 0.0, rw = 1.0, lw = 0.0, fw = 0.5, mw = 0.5, cw = 0.1, phase_ratio = 0.3, strict_cut = 0.30, soft_cut = 0.36;
  bool has_latent() const { return lw != 0.0; }
};
// the argument checks of the loss setters and entry points: JAT_OK, or JAT_E_INVALID with its text set
int check_band_ratios(const LossSpec& l), check_recon_eps(const LossSpec& l), check_loss_weights(const LossSpec& l);
// One loss launch on [rows, T], host arithmetic only (ratios that passed check_band_ratios): the latent kernels (they hold the
// reconstruction term too) or the reconstruction kernel alone; band edges in rfft bins; the latent kernels' path at T; scratch bytes:
// recon = train_red_blocks() partial sums + the 2-float result, latent = tw_bytes ([T] twiddles padded to 256 B) + rows * 8 partials
struct LossLaunch { bool latent; int low, strict, soft; LatentLossPlan path; size_t recon_bytes, tw_bytes, latent_bytes; };
LossLaunch plan_loss(const LossSpec& l, int64_t rows, int T);
std::vector<float2> make_twiddles(int T);   // (cos, sin)(2 pi i / T)
// The one place a loss is launched: dpred = d(loss * loss_scale)/d pred and out = {rw * recon, scratch} (reconstruction; lr, tw unused)
// or the six terms {total, recon, freq, ms, cons, latent} (latent; lr may be null when cw == 0); part: the family's partial sums
int run_loss(const LossSpec& l, const LossLaunch& p, const float* pred, const float* target, const float* lr, const float2* tw,
             float* dpred, float* part, float* out, int64_t rows, int T, float loss_scale, hipStream_t s);
