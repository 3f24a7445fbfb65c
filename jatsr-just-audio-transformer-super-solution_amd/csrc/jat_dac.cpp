// C ABI of the DAC 44.1 kHz decoder (include/jat_hip.h): weight preparation at create, the stage chain of decode.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "jat_dac_kernels.h"
#include "jat_internal.h"

namespace {

uint16_t host_bf16(float f) {   // round-to-nearest-even (finite inputs)
  uint32_t u;
  std::memcpy(&u, &f, 4);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
float host_bf2f(uint16_t h) {
  const uint32_t u = (uint32_t)h << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

// torch layout -> [N, taps, cin]
void pack(int kind, const float* w, int cin, int cout, int ks, std::vector<float>& out) {
  if (kind == 2) {
    // strided Conv1d [cout, cin, 2s], padding s/2, over super-rows of s input rows ([T_in, cin] read as [T_in/s, s*cin]):
    // output t reads super-rows t - 1 + j (j < 3); row u of super-row j is input t*s + (j-1)*s + u, tap
    // k = (j-1)*s + u + s/2 when 0 <= k < 2s (torch: i = t*s - pad + k), zero otherwise.  Result [cout, 3, s*cin].
    const int s = ks, p = s / 2;
    out.assign((size_t)cout * 3 * s * cin, 0.f);
    for (int co = 0; co < cout; ++co)
      for (int j = 0; j < 3; ++j)
        for (int u = 0; u < s; ++u) {
          const int k = (j - 1) * s + u + p;
          if (k < 0 || k >= 2 * s) continue;
          for (int ci = 0; ci < cin; ++ci)
            out[(((size_t)co * 3 + j) * s + u) * cin + ci] = w[((size_t)co * cin + ci) * 2 * s + k];
        }
    return;
  }
  if (kind == 0) {   // Conv1d [cout, cin, k]
    out.assign((size_t)cout * ks * cin, 0.f);
    for (int co = 0; co < cout; ++co)
      for (int ci = 0; ci < cin; ++ci)
        for (int k = 0; k < ks; ++k) out[((size_t)co * ks + k) * cin + ci] = w[((size_t)co * cin + ci) * ks + k];
    return;
  }
  // ConvTranspose1d [cin, cout, 2s], padding s/2: output o = q*s + r reads input q + shift (shift = j - 1) through tap
  // k = r + s/2 - shift*s when 0 <= k < 2s (torch: o = i*s - pad + k)
  const int s = ks, p = s / 2;
  out.assign((size_t)s * cout * 3 * cin, 0.f);
  for (int r = 0; r < s; ++r)
    for (int j = 0; j < 3; ++j) {
      const int k = r + p - (j - 1) * s;
      if (k < 0 || k >= 2 * s) continue;
      for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
          out[(((size_t)r * cout + co) * 3 + j) * cin + ci] = w[((size_t)ci * cout + co) * 2 * s + k];
    }
}

struct DacConv {
  int taps = 0, dil = 1, cin = 0, cout = 0, N = 0;
  uint16_t *w_hi = nullptr, *w_lo = nullptr;
  float* bias = nullptr;
};
struct DacUnit {
  float *a1 = nullptr, *a2 = nullptr;
  DacConv c1, c2;
};
struct DacBlock {
  float* a_in = nullptr;
  DacConv ct;
  DacUnit u[3];
  int stride = 0;
};

int check_dims(const jat_dac_config& c) {
  if (c.latent_channels <= 0 || c.latent_channels % 32) return fail(JAT_E_INVALID, "dac: latent_channels %d is not a multiple of 32", c.latent_channels);
  if (c.n_blocks < 1 || c.n_blocks > 4) return fail(JAT_E_INVALID, "dac: n_blocks %d not in 1..4", c.n_blocks);
  for (int i = 0; i <= c.n_blocks; ++i)
    if (c.channels <= 0 || (c.channels >> i) % 32 || (c.channels >> i) << i != c.channels)
      return fail(JAT_E_INVALID, "dac: channels %d >> %d is not a multiple of 32", c.channels, i);
  if ((c.channels >> c.n_blocks) > 96) return fail(JAT_E_INVALID, "dac: tail channels %d > 96", c.channels >> c.n_blocks);
  for (int i = 0; i < c.n_blocks; ++i)
    if (c.strides[i] < 2 || c.strides[i] % 2) return fail(JAT_E_INVALID, "dac: stride %d of block %d is not even", c.strides[i], i);
  return JAT_OK;
}

int conv_args_check(int32_t cin, int32_t N, int32_t cch, int32_t taps, int32_t dil, int32_t precision) {
  if (cin <= 0 || cin % 32) return fail(JAT_E_INVALID, "dac conv: cin %d is not a multiple of 32", cin);
  if (cch <= 0 || cch % 32 || N <= 0 || N % cch) return fail(JAT_E_INVALID, "dac conv: N %d / cch %d not multiples of 32", N, cch);
  if (!(taps == 7 && dil >= 1 && dil <= DAC_MAX_DIL) && !((taps == 3 || taps == 1) && dil == 1))
    return fail(JAT_E_INVALID, "dac conv: taps %d dilation %d unsupported", taps, dil);
  if (precision != JAT_DAC_BF16X3 && precision != JAT_DAC_BF16) return fail(JAT_E_INVALID, "dac: precision %d", precision);
  return JAT_OK;
}

}  // namespace

struct jat_dac_decoder {
  jat_dac_config cfg{};
  int max_B = 0, max_T = 0, hop = 1;
  DacConv conv1;
  DacBlock blk[4];
  float *a_out = nullptr, *tail_w = nullptr, *tail_b = nullptr;
  uint16_t *P[2] = {nullptr, nullptr}, *Q[2] = {nullptr, nullptr};   // operand planes (hi, lo), ping-pong
  float* X = nullptr;                                                // fp32 residual stream
  size_t bytes = 0;
  std::vector<void*> allocs;
  ~jat_dac_decoder() {
    for (void* p : allocs) (void)hipFree(p);
  }
  int alloc(void** p, size_t n) {
    n = align_up(n < 16 ? 16 : n, 256);
    HIPCHK(hipMalloc(p, n));
    allocs.push_back(*p);
    bytes += n;
    return JAT_OK;
  }
};

namespace {

struct Named {
  const jat_tensor_ref* refs;
  int n;
  int get(const std::string& key, int64_t numel, std::vector<float>& host) const {
    for (int i = 0; i < n; ++i)
      if (refs[i].name && key == refs[i].name) {
        if (refs[i].numel != numel)
          return fail(JAT_E_INVALID, "dac: parameter %s has %lld elements, expected %lld", key.c_str(), (long long)refs[i].numel,
                      (long long)numel);
        host.resize(numel);
        HIPCHK(hipMemcpy(host.data(), refs[i].data, numel * sizeof(float), hipMemcpyDeviceToHost));
        return JAT_OK;
      }
    return fail(JAT_E_INVALID, "dac: missing parameter %s", key.c_str());
  }
};

template <class H>
int upload(H* d, const std::vector<float>& h, float** out) {
  JCHK(d->alloc((void**)out, h.size() * sizeof(float)));
  HIPCHK(hipMemcpy(*out, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
  return JAT_OK;
}

// kind 0 Conv1d k = ks, 1 ConvTranspose1d stride ks, 2 strided Conv1d stride ks (super-rows: the GEMM's cin is ks * cin)
template <class H>
int load_conv(H* d, const Named& nm, const std::string& pre, int kind, int cin, int cout, int ks, int dil, DacConv& c) {
  std::vector<float> w, b, packed;
  JCHK(nm.get(pre + ".weight", (int64_t)cin * cout * (kind != 0 ? 2 * ks : ks), w));
  JCHK(nm.get(pre + ".bias", cout, b));
  pack(kind, w.data(), cin, cout, ks, packed);
  c.taps = kind != 0 ? 3 : ks;
  c.dil = dil;
  c.cin = kind == 2 ? ks * cin : cin;
  c.cout = cout;
  c.N = kind == 1 ? ks * cout : cout;
  std::vector<uint16_t> hi(packed.size()), lo(packed.size());
  for (size_t i = 0; i < packed.size(); ++i) {
    hi[i] = host_bf16(packed[i]);
    lo[i] = host_bf16(packed[i] - host_bf2f(hi[i]));
  }
  JCHK(d->alloc((void**)&c.w_hi, hi.size() * 2));
  JCHK(d->alloc((void**)&c.w_lo, lo.size() * 2));
  HIPCHK(hipMemcpy(c.w_hi, hi.data(), hi.size() * 2, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(c.w_lo, lo.data(), lo.size() * 2, hipMemcpyHostToDevice));
  return upload(d, b, &c.bias);
}

template <class H>
int load_alpha(H* d, const Named& nm, const std::string& key, int ch, float** out) {
  std::vector<float> a;
  JCHK(nm.get(key, ch, a));
  return upload(d, a, out);
}

int run_conv(const DacConv& c, const uint16_t* const* A, const float* res, float* out32, const float* alpha, uint16_t* const* O,
             int B, int T, bool x3, hipStream_t s) {
  DacConvArgs p{};
  p.a_hi = A[0], p.a_lo = A[1], p.w_hi = c.w_hi, p.w_lo = c.w_lo, p.bias = c.bias, p.res = res, p.out32 = out32;
  p.alpha = alpha, p.o_hi = O ? O[0] : nullptr, p.o_lo = O ? O[1] : nullptr;
  p.M = (int64_t)B * T, p.T = T, p.Cin = c.cin, p.N = c.N, p.Cch = c.cout, p.dil = c.dil;
  KCHK(dac_launch_conv(p, c.taps, x3, s));
  return JAT_OK;
}

}  // namespace

extern "C" int jat_dac_decoder_create(const jat_dac_config* cfg, const jat_tensor_ref* named, int32_t n, int32_t max_B,
                                      int32_t max_T, void* stream, jat_dac_decoder** out) {
  if (!cfg || !out || (n > 0 && !named)) return fail(JAT_E_INVALID, "dac: null argument");
  *out = nullptr;
  JCHK(check_dims(*cfg));
  if (max_B < 1 || max_T < 1) return fail(JAT_E_INVALID, "dac: max_B %d / max_T %d must be >= 1", max_B, max_T);
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));   // the named tensors may have been written on this stream
  std::unique_ptr<jat_dac_decoder> d(new jat_dac_decoder());
  d->cfg = *cfg;
  d->max_B = max_B, d->max_T = max_T;
  const Named nm{named, n};
  const int C0 = cfg->channels;
  // modeling_dac.py:416: conv1 = Conv1d(hidden_size, channels, k7, p3)
  JCHK(load_conv(d.get(), nm, "conv1", 0, cfg->latent_channels, C0, 7, 1, d->conv1));
  const int64_t BT = (int64_t)max_B * max_T;
  int64_t op_elems = BT * std::max(cfg->latent_channels, C0), x_elems = 0, rows = BT;
  for (int i = 0; i < cfg->n_blocks; ++i) {   // modeling_dac.py:236-264
    const int s = cfg->strides[i], cin = C0 >> i, cout = C0 >> (i + 1);
    const std::string pre = "block." + std::to_string(i);
    DacBlock& b = d->blk[i];
    b.stride = s;
    JCHK(load_alpha(d.get(), nm, pre + ".snake1.alpha", cin, &b.a_in));
    JCHK(load_conv(d.get(), nm, pre + ".conv_t1", 1, cin, cout, s, 1, b.ct));
    const int dil[3] = {1, 3, 9};
    for (int u = 0; u < 3; ++u) {
      const std::string ru = pre + ".res_unit" + std::to_string(u + 1);
      JCHK(load_alpha(d.get(), nm, ru + ".snake1.alpha", cout, &b.u[u].a1));
      JCHK(load_conv(d.get(), nm, ru + ".conv1", 0, cout, cout, 7, dil[u], b.u[u].c1));
      JCHK(load_alpha(d.get(), nm, ru + ".snake2.alpha", cout, &b.u[u].a2));
      JCHK(load_conv(d.get(), nm, ru + ".conv2", 0, cout, cout, 1, 1, b.u[u].c2));
    }
    rows *= s;
    op_elems = std::max(op_elems, rows * cout);
    x_elems = std::max(x_elems, rows * cout);
    d->hop *= s;
  }
  const int Cf = C0 >> cfg->n_blocks;
  JCHK(load_alpha(d.get(), nm, "snake1.alpha", Cf, &d->a_out));   // modeling_dac.py:423-425
  {
    std::vector<float> w, b;
    JCHK(nm.get("conv2.weight", (int64_t)Cf * 7, w));
    JCHK(nm.get("conv2.bias", 1, b));
    std::vector<float> wt((size_t)7 * Cf);
    for (int ci = 0; ci < Cf; ++ci)
      for (int k = 0; k < 7; ++k) wt[(size_t)k * Cf + ci] = w[(size_t)ci * 7 + k];
    JCHK(upload(d.get(), wt, &d->tail_w));
    JCHK(upload(d.get(), b, &d->tail_b));
  }
  for (int h = 0; h < 2; ++h) {
    JCHK(d->alloc((void**)&d->P[h], op_elems * 2));
    JCHK(d->alloc((void**)&d->Q[h], op_elems * 2));
  }
  JCHK(d->alloc((void**)&d->X, x_elems * 4));
  *out = d.release();
  return JAT_OK;
}

extern "C" void jat_dac_decoder_destroy(jat_dac_decoder* d) { delete d; }

extern "C" int jat_dac_workspace_bytes(const jat_dac_decoder* d, size_t* bytes) {
  if (!d || !bytes) return fail(JAT_E_INVALID, "dac: null argument");
  *bytes = d->bytes;
  return JAT_OK;
}

extern "C" int jat_dac_decode(jat_dac_decoder* d, const float* z, float* audio, int32_t B, int32_t T, int32_t precision,
                              void* stream) {
  if (!d || !z || !audio) return fail(JAT_E_INVALID, "dac: null argument");
  if (B < 1 || B > d->max_B) return fail(JAT_E_INVALID, "dac: B = %d outside 1..max_B = %d", B, d->max_B);
  if (T < 1 || T > d->max_T) return fail(JAT_E_INVALID, "dac: T = %d outside 1..max_T = %d", T, d->max_T);
  if (precision != JAT_DAC_BF16X3 && precision != JAT_DAC_BF16) return fail(JAT_E_INVALID, "dac: precision %d", precision);
  const hipStream_t s = (hipStream_t)stream;
  const bool x3 = precision == JAT_DAC_BF16X3;
  uint16_t** cur = d->Q;   // the operand of the next conv
  uint16_t** nxt = d->P;
  KCHK(dac_launch_z_split(z, cur[0], x3 ? cur[1] : nullptr, B, d->cfg.latent_channels, T, s));
  // conv1 (modeling_dac.py:428); its output feeds block 0's snake1 only
  JCHK(run_conv(d->conv1, cur, nullptr, nullptr, d->blk[0].a_in, nxt, B, T, x3, s));
  std::swap(cur, nxt);
  int Tc = T;
  for (int i = 0; i < d->cfg.n_blocks; ++i) {
    DacBlock& b = d->blk[i];
    // snake1 -> conv_t1 (modeling_dac.py:259-260): the fp32 output starts the residual stream, its snake feeds res_unit1
    JCHK(run_conv(b.ct, cur, nullptr, d->X, b.u[0].a1, nxt, B, Tc, x3, s));
    std::swap(cur, nxt);
    Tc *= b.stride;
    for (int u = 0; u < 3; ++u) {   // modeling_dac.py:196-209, 261-263
      JCHK(run_conv(b.u[u].c1, cur, nullptr, nullptr, b.u[u].a2, nxt, B, Tc, x3, s));
      std::swap(cur, nxt);
      const bool last = i + 1 == d->cfg.n_blocks && u == 2;
      const float* a_next = u < 2 ? b.u[u + 1].a1 : (last ? nullptr : d->blk[i + 1].a_in);
      JCHK(run_conv(b.u[u].c2, cur, d->X, d->X, a_next, last ? nullptr : nxt, B, Tc, x3, s));
      std::swap(cur, nxt);
    }
  }
  // snake1 -> conv2 -> tanh (modeling_dac.py:436-439)
  KCHK(dac_launch_tail(d->X, d->a_out, d->tail_w, d->tail_b, audio, d->cfg.channels >> d->cfg.n_blocks, Tc, (int64_t)B * Tc, s));
  return JAT_OK;
}

extern "C" int jat_dac_pack_weight(int32_t kind, const float* w, int32_t cin, int32_t cout, int32_t k_or_stride, float* out) {
  if (!w || !out || cin < 1 || cout < 1 || k_or_stride < 1) return fail(JAT_E_INVALID, "dac pack: bad argument");
  if (kind != 0 && k_or_stride % 2) return fail(JAT_E_INVALID, "dac pack: odd stride %d", k_or_stride);
  if (kind < 0 || kind > 2) return fail(JAT_E_INVALID, "dac pack: kind %d", kind);
  std::vector<float> v;
  pack(kind, w, cin, cout, k_or_stride, v);
  std::memcpy(out, v.data(), v.size() * sizeof(float));
  return JAT_OK;
}

extern "C" int jat_k_dac_split(const float* x, uint16_t* hi, uint16_t* lo, int64_t n, void* stream) {
  KCHK(dac_launch_split(x, hi, lo, n, (hipStream_t)stream));
  return JAT_OK;
}

extern "C" int jat_k_dac_conv(const uint16_t* a_hi, const uint16_t* a_lo, const uint16_t* w_hi, const uint16_t* w_lo,
                              const float* bias, const float* res, float* out32, const float* alpha, uint16_t* o_hi,
                              uint16_t* o_lo, int32_t B, int32_t T, int32_t cin, int32_t N, int32_t cch, int32_t taps,
                              int32_t dil, int32_t precision, void* stream) {
  JCHK(conv_args_check(cin, N, cch, taps, dil, precision));
  if (B < 1 || T < 1) return fail(JAT_E_INVALID, "dac conv: B %d T %d", B, T);
  if (o_hi && !alpha) return fail(JAT_E_INVALID, "dac conv: snake output without alpha");
  const bool x3 = precision == JAT_DAC_BF16X3;
  if (x3 && (!a_lo || !w_lo || (o_hi && !o_lo))) return fail(JAT_E_INVALID, "dac conv: bf16x3 needs the lo planes");
  DacConvArgs p{};
  p.a_hi = a_hi, p.a_lo = a_lo, p.w_hi = w_hi, p.w_lo = w_lo, p.bias = bias, p.res = res, p.out32 = out32;
  p.alpha = alpha, p.o_hi = o_hi, p.o_lo = o_lo;
  p.M = (int64_t)B * T, p.T = T, p.Cin = cin, p.N = N, p.Cch = cch, p.dil = dil;
  KCHK(dac_launch_conv(p, taps, x3, (hipStream_t)stream));
  return JAT_OK;
}

extern "C" int jat_k_dac_tail(const float* x, const float* alpha, const float* w, const float* bias, float* out, int32_t B,
                              int32_t T, int32_t C, void* stream) {
  if (B < 1 || T < 1 || C < 1 || C > 96) return fail(JAT_E_INVALID, "dac tail: B %d T %d C %d", B, T, C);
  KCHK(dac_launch_tail(x, alpha, w, bias, out, C, T, (int64_t)B * T, (hipStream_t)stream));
  return JAT_OK;
}

// ---- encoder ------------------------------------------------------------------------------------------------------------
namespace {

struct DacEncUnit {
  float *a1 = nullptr, *a2 = nullptr;
  DacConv c1, c2;
};
struct DacEncBlock {
  DacEncUnit u[3];
  float* a_down = nullptr;   // block snake1, the operand of the strided conv
  DacConv down;
  int stride = 0;
};

int check_enc_dims(const jat_dac_encoder_config& c) {
  if (c.channels <= 0 || c.channels % 32) return fail(JAT_E_INVALID, "dac encoder: channels %d is not a multiple of 32", c.channels);
  if (c.n_blocks < 1 || c.n_blocks > 4) return fail(JAT_E_INVALID, "dac encoder: n_blocks %d not in 1..4", c.n_blocks);
  for (int i = 0; i < c.n_blocks; ++i)
    if (c.strides[i] < 2 || c.strides[i] % 2) return fail(JAT_E_INVALID, "dac encoder: stride %d of block %d is not even", c.strides[i], i);
  if ((int64_t)c.channels << c.n_blocks > 8192) return fail(JAT_E_INVALID, "dac encoder: channels %d << %d too wide", c.channels, c.n_blocks);
  if (c.hidden_size != 1024 || c.codebook_size != 1024 || c.codebook_dim != 8)
    return fail(JAT_E_INVALID, "dac encoder: the RVQ kernel takes hidden_size 1024 and 1024 x 8 codebooks, got %d, %d x %d",
                c.hidden_size, c.codebook_size, c.codebook_dim);
  if (c.n_codebooks < 1 || c.n_codebooks > JAT_DAC_MAX_CODEBOOKS)
    return fail(JAT_E_INVALID, "dac encoder: n_codebooks %d not in 1..%d", c.n_codebooks, JAT_DAC_MAX_CODEBOOKS);
  return JAT_OK;
}

}  // namespace

struct jat_dac_encoder {
  jat_dac_encoder_config cfg{};
  int max_B = 0, max_T = 0, hop = 1;
  float *head_w = nullptr, *head_b = nullptr;
  DacEncBlock blk[4];
  float* a_final = nullptr;   // encoder.snake1
  DacConv conv2;
  float *w_in = nullptr, *b_in = nullptr, *cb = nullptr, *w_out = nullptr, *b_out = nullptr;   // [n_codebooks, ...]
  uint16_t *P[2] = {nullptr, nullptr}, *Q[2] = {nullptr, nullptr};   // operand planes (hi, lo), ping-pong
  float* X = nullptr;   // fp32 residual stream; after conv2 the encoder output [B*T, hidden] channels-last
  size_t bytes = 0;
  std::vector<void*> allocs;
  ~jat_dac_encoder() {
    for (void* p : allocs) (void)hipFree(p);
  }
  int alloc(void** p, size_t n) {
    n = align_up(n < 16 ? 16 : n, 256);
    HIPCHK(hipMalloc(p, n));
    allocs.push_back(*p);
    bytes += n;
    return JAT_OK;
  }
};

extern "C" int jat_dac_encoder_create(const jat_dac_encoder_config* cfg, const jat_tensor_ref* named, int32_t n,
                                      int32_t max_B, int32_t max_T, void* stream, jat_dac_encoder** out) {
  if (!cfg || !out || (n > 0 && !named)) return fail(JAT_E_INVALID, "dac encoder: null argument");
  *out = nullptr;
  JCHK(check_enc_dims(*cfg));
  if (max_B < 1 || max_T < 1) return fail(JAT_E_INVALID, "dac encoder: max_B %d / max_T %d must be >= 1", max_B, max_T);
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));   // the named tensors may have been written on this stream
  std::unique_ptr<jat_dac_encoder> d(new jat_dac_encoder());
  d->cfg = *cfg;
  d->max_B = max_B, d->max_T = max_T;
  const Named nm{named, n};
  const int C0 = cfg->channels;
  {   // modeling_dac.py:450: conv1 = Conv1d(1, C0, k7, p3), kept in torch layout [C0, 1, 7] for the head kernel
    std::vector<float> w, b;
    JCHK(nm.get("encoder.conv1.weight", (int64_t)C0 * 7, w));
    JCHK(nm.get("encoder.conv1.bias", C0, b));
    JCHK(upload(d.get(), w, &d->head_w));
    JCHK(upload(d.get(), b, &d->head_b));
  }
  for (int i = 0; i < cfg->n_blocks; ++i) {   // modeling_dac.py:212-234
    const int s = cfg->strides[i], c = C0 << i;
    const std::string pre = "encoder.block." + std::to_string(i);
    DacEncBlock& b = d->blk[i];
    b.stride = s;
    d->hop *= s;
    const int dil[3] = {1, 3, 9};
    for (int u = 0; u < 3; ++u) {
      const std::string ru = pre + ".res_unit" + std::to_string(u + 1);
      JCHK(load_alpha(d.get(), nm, ru + ".snake1.alpha", c, &b.u[u].a1));
      JCHK(load_conv(d.get(), nm, ru + ".conv1", 0, c, c, 7, dil[u], b.u[u].c1));
      JCHK(load_alpha(d.get(), nm, ru + ".snake2.alpha", c, &b.u[u].a2));
      JCHK(load_conv(d.get(), nm, ru + ".conv2", 0, c, c, 1, 1, b.u[u].c2));
    }
    JCHK(load_alpha(d.get(), nm, pre + ".snake1.alpha", c, &b.a_down));
    JCHK(load_conv(d.get(), nm, pre + ".conv1", 2, c, 2 * c, s, 1, b.down));
  }
  const int Cf = C0 << cfg->n_blocks, H = cfg->hidden_size, NQ = cfg->n_codebooks;
  JCHK(load_alpha(d.get(), nm, "encoder.snake1.alpha", Cf, &d->a_final));   // modeling_dac.py:458-461
  JCHK(load_conv(d.get(), nm, "encoder.conv2", 0, Cf, H, 3, 1, d->conv2));
  {   // quantizer.quantizers.{i}: in_proj [8, H, 1], out_proj [H, 8, 1], codebook [1024, 8], stacked over i
    const int CD = cfg->codebook_dim, NC = cfg->codebook_size;
    std::vector<float> w_in, b_in, cb, w_out, b_out, t;
    for (int i = 0; i < NQ; ++i) {
      const std::string pre = "quantizer.quantizers." + std::to_string(i);
      JCHK(nm.get(pre + ".in_proj.weight", (int64_t)CD * H, t));
      w_in.insert(w_in.end(), t.begin(), t.end());
      JCHK(nm.get(pre + ".in_proj.bias", CD, t));
      b_in.insert(b_in.end(), t.begin(), t.end());
      JCHK(nm.get(pre + ".codebook.weight", (int64_t)NC * CD, t));
      cb.insert(cb.end(), t.begin(), t.end());
      JCHK(nm.get(pre + ".out_proj.weight", (int64_t)H * CD, t));
      w_out.insert(w_out.end(), t.begin(), t.end());
      JCHK(nm.get(pre + ".out_proj.bias", H, t));
      b_out.insert(b_out.end(), t.begin(), t.end());
    }
    JCHK(upload(d.get(), w_in, &d->w_in));
    JCHK(upload(d.get(), b_in, &d->b_in));
    JCHK(upload(d.get(), cb, &d->cb));
    JCHK(upload(d.get(), w_out, &d->w_out));
    JCHK(upload(d.get(), b_out, &d->b_out));
  }
  // Every stage holds rows * channels <= B * T * hop * C0 elements (channels double at most as fast as the stride divides
  // the rows); the encoder output [B*T, H] fits there as well.
  const int64_t rows = (int64_t)max_B * max_T * d->hop;
  const int64_t elems = std::max(rows * C0, (int64_t)max_B * max_T * H);
  for (int h = 0; h < 2; ++h) {
    JCHK(d->alloc((void**)&d->P[h], elems * 2));
    JCHK(d->alloc((void**)&d->Q[h], elems * 2));
  }
  JCHK(d->alloc((void**)&d->X, elems * 4));
  *out = d.release();
  return JAT_OK;
}

extern "C" void jat_dac_encoder_destroy(jat_dac_encoder* d) { delete d; }

extern "C" int jat_dac_encoder_workspace_bytes(const jat_dac_encoder* d, size_t* bytes) {
  if (!d || !bytes) return fail(JAT_E_INVALID, "dac encoder: null argument");
  *bytes = d->bytes;
  return JAT_OK;
}

extern "C" int jat_dac_encode(jat_dac_encoder* d, const float* audio, float* z, int32_t* codes, float* latents,
                              float* hidden, int32_t B, int32_t T, int32_t n_quantizers, int32_t precision, void* stream) {
  if (!d || !audio || !z) return fail(JAT_E_INVALID, "dac encoder: null argument");
  if (B < 1 || B > d->max_B) return fail(JAT_E_INVALID, "dac encoder: B = %d outside 1..max_B = %d", B, d->max_B);
  if (T < 1 || T > d->max_T) return fail(JAT_E_INVALID, "dac encoder: T = %d outside 1..max_T = %d", T, d->max_T);
  if (n_quantizers < 1 || n_quantizers > d->cfg.n_codebooks)
    return fail(JAT_E_INVALID, "dac encoder: n_quantizers %d outside 1..%d", n_quantizers, d->cfg.n_codebooks);
  if (precision != JAT_DAC_BF16X3 && precision != JAT_DAC_BF16) return fail(JAT_E_INVALID, "dac encoder: precision %d", precision);
  const hipStream_t s = (hipStream_t)stream;
  const bool x3 = precision == JAT_DAC_BF16X3;
  uint16_t** cur = d->Q;   // the operand of the next conv
  uint16_t** nxt = d->P;
  int Tc = T * d->hop;
  // conv1 (modeling_dac.py:467): the fp32 output starts block 0's residual stream, its snake feeds res_unit1
  KCHK(dac_launch_head(audio, d->head_w, d->head_b, d->blk[0].u[0].a1, d->X, cur[0], x3 ? cur[1] : nullptr, d->cfg.channels,
                       Tc, (int64_t)B * Tc, s));
  for (int i = 0; i < d->cfg.n_blocks; ++i) {
    DacEncBlock& b = d->blk[i];
    for (int u = 0; u < 3; ++u) {   // modeling_dac.py:196-209, 229-231
      JCHK(run_conv(b.u[u].c1, cur, nullptr, nullptr, b.u[u].a2, nxt, B, Tc, x3, s));
      std::swap(cur, nxt);
      JCHK(run_conv(b.u[u].c2, cur, d->X, d->X, u < 2 ? b.u[u + 1].a1 : b.a_down, nxt, B, Tc, x3, s));
      std::swap(cur, nxt);
    }
    // snake1 -> strided conv1 (modeling_dac.py:231-232) on super-rows; its fp32 output starts the next block's stream
    Tc /= b.stride;
    const bool last = i + 1 == d->cfg.n_blocks;
    JCHK(run_conv(b.down, cur, nullptr, last ? nullptr : d->X, last ? d->a_final : d->blk[i + 1].u[0].a1, nxt, B, Tc, x3, s));
    std::swap(cur, nxt);
  }
  // snake1 -> conv2 (modeling_dac.py:472-473) -> the quantizer's input, fp32 channels-last
  JCHK(run_conv(d->conv2, cur, nullptr, d->X, nullptr, nullptr, B, T, x3, s));
  DacRvqArgs p{};
  p.hidden = d->X, p.w_in = d->w_in, p.b_in = d->b_in, p.codebook = d->cb, p.w_out = d->w_out, p.b_out = d->b_out;
  p.z = z, p.codes = codes, p.latents = latents, p.hidden_cm = hidden;
  p.M = (int64_t)B * T, p.T = T, p.nq = n_quantizers;
  KCHK(dac_launch_rvq(p, s));
  return JAT_OK;
}

extern "C" int jat_k_dac_head(const float* audio, const float* w, const float* bias, const float* alpha, float* out32,
                              uint16_t* o_hi, uint16_t* o_lo, int32_t B, int32_t L, int32_t C, void* stream) {
  if (B < 1 || L < 1 || C < 32 || C % 32 || C > 8192) return fail(JAT_E_INVALID, "dac head: B %d L %d C %d", B, L, C);
  if (!audio || !w || !bias) return fail(JAT_E_INVALID, "dac head: null argument");
  if (o_hi && !alpha) return fail(JAT_E_INVALID, "dac head: snake output without alpha");
  KCHK(dac_launch_head(audio, w, bias, alpha, out32, o_hi, o_lo, C, L, (int64_t)B * L, (hipStream_t)stream));
  return JAT_OK;
}

extern "C" int jat_k_dac_rvq(const float* hidden, const float* w_in, const float* b_in, const float* codebook,
                             const float* w_out, const float* b_out, float* z, int32_t* codes, float* latents,
                             float* hidden_cm, int32_t B, int32_t T, int32_t hidden_size, int32_t n_quantizers,
                             void* stream) {
  if (B < 1 || T < 1) return fail(JAT_E_INVALID, "dac rvq: B %d T %d", B, T);
  if (hidden_size != 1024) return fail(JAT_E_INVALID, "dac rvq: hidden_size %d (the kernel takes 1024)", hidden_size);
  if (n_quantizers < 1 || n_quantizers > JAT_DAC_MAX_CODEBOOKS)
    return fail(JAT_E_INVALID, "dac rvq: n_quantizers %d outside 1..%d", n_quantizers, JAT_DAC_MAX_CODEBOOKS);
  if (!hidden || !w_in || !b_in || !codebook || !w_out || !b_out || !z) return fail(JAT_E_INVALID, "dac rvq: null argument");
  DacRvqArgs p{};
  p.hidden = hidden, p.w_in = w_in, p.b_in = b_in, p.codebook = codebook, p.w_out = w_out, p.b_out = b_out;
  p.z = z, p.codes = codes, p.latents = latents, p.hidden_cm = hidden_cm;
  p.M = (int64_t)B * T, p.T = T, p.nq = n_quantizers;
  KCHK(dac_launch_rvq(p, (hipStream_t)stream));
  return JAT_OK;
}
