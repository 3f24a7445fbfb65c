"""Plain torch-fp64 restatement of the DiT forward with STATED ROUNDING POINTS — test infrastructure.

Every function takes `rnd`: the identity, or "round to the library's operand dtype and back to fp64" (`make_rnd`).  With the
identity the twin is `oracle.jat_oracle.OracleModel` in fp64 (tests/test_forward_ref_cpu.py: 1e-12); with the operand
rounding it rounds exactly where DESIGN.md §2/§3 say the HIP path does, and nowhere else:

    rounded   GEMM weights (adaLN's among them: they are packed with the others, §3) and silu(t_emb), adaLN's A operand;
              the normalised + modulated row that feeds qkv, fc1 and the final linear; q and k after RoPE, and v; the
              un-normalised softmax probabilities before PV; the attention output; the GELU output; the patchified input
              and the patch-embed hidden
    fp64      the residual stream, norm statistics, softmax maxima and sums, RoPE angles (the oracle's fp32 tables),
              the modulation vectors themselves, biases, the time MLP, the sampler state

`fold=True` moves the rounding points to where the sampler's folded norms have them: the A operand of qkv /
fc1 / the final linear is the rounded residual row itself, the weight is rnd(W diag(w_norm (1 + scale))), the row's rstd
multiplies the accumulator, the shift enters as rnd(shift) @ rnd(W)^T, and the residual stream lives as two rounded planes
hi + lo.  With the identity, fold=True computes the same function as fold=False.

The code is device-agnostic torch: the CPU tests pin it to the oracle on the CPU, the GPU tests evaluate the very same
functions in fp64 on the device (`Twin(device="cuda")`), as tests/test_gpu_kernels.py does for its per-kernel references.

The error of twin(rnd) against twin(identity) on the same inputs, `E0`, is a property of this file alone; the GPU tests
(tests/test_gpu_forward_paths.py) gate the kernels on a small multiple of it.
"""
import math

import numpy as np
import torch

F64 = torch.float64
HEAD_DIM = 64


def identity(t):
    return t


def make_rnd(dtype):
    """round to `dtype` (torch.bfloat16 / torch.float16; None = identity) and back to fp64"""
    if dtype is None:
        return identity
    return lambda t: t.to(dtype).to(F64)


def t64(a):
    return torch.as_tensor(np.asarray(a)).to(F64) if not torch.is_tensor(a) else a.to(F64)


def rel_l2(a, b):
    a, b = t64(a), t64(b)
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


# ---- elementary ops -------------------------------------------------------------------------------------------------------
def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def silu(x):
    return x / (1.0 + torch.exp(-x))


def norm_rows(x, weight, mode):
    """RMSNorm(eps=1e-6) with weight (mode 'rms') or LayerNorm without affine (mode 'ln'), statistics in fp64"""
    if mode == "rms":
        y = x / torch.sqrt((x * x).mean(-1, keepdim=True) + 1e-6)
        return y * weight if weight is not None else y
    mu = x.mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + 1e-6)


def rope_inv_freq(head_dim=HEAD_DIM, base=10000.0):
    """inv_freq[i] = base^(-2i/head_dim), fp32 arithmetic as the reference's RoPE buffers"""
    return (np.float32(1.0) / (np.float32(base) ** (np.arange(0, head_dim, 2, dtype=np.float32) / np.float32(head_dim)))).astype(
        np.float32)


def rope_tables(n, inv_freq=None):
    """cos / sin [n, head_dim]: fp32 angles and fp32 cos / sin as the reference builds its buffers, carried in fp64"""
    inv_freq = rope_inv_freq() if inv_freq is None else np.asarray(inv_freq, np.float32)
    freqs = np.outer(np.arange(n, dtype=np.float32), inv_freq).astype(np.float32)
    emb = np.concatenate([freqs, freqs], -1)
    return torch.from_numpy(np.cos(emb)).to(F64), torch.from_numpy(np.sin(emb)).to(F64)


def apply_rope(x, cos, sin):
    """x [B, N, H, hd]; rotate-half form"""
    h = x.shape[-1] // 2
    rot = torch.cat([-x[..., h:], x[..., :h]], -1)
    return x * cos[None, :, None, :] + rot * sin[None, :, None, :]


def time_embedding(t, dim):
    half = dim // 2
    k = math.log(10000) / (half - 1)
    freqs = torch.from_numpy(np.exp(np.arange(half, dtype=np.float32) * np.float32(-k))).to(t.device, F64)
    e = t[:, None] * freqs[None, :]
    return torch.cat([torch.sin(e), torch.cos(e)], -1)


def linspace_f32(a, b, n):
    """torch.linspace(a, b, n) in fp32: each value rounded once"""
    a32, b32 = np.float32(a), np.float32(b)
    step = float(np.float32((b32 - a32) / np.float32(n - 1)))
    return np.array([np.float32(float(a32) + step * i) if i < n // 2 else np.float32(float(b32) - step * (n - 1 - i))
                     for i in range(n)], np.float32)


# ---- the attention kernels' operation on its own ---------------------------------------------------------------------------
def attention_heads(q, k, v, B, N, Hq, Hkv, lens=None):
    """softmax(q k^T / 8) v with GQA head sharing in fp64, on operands as the kernels get them: q [B*N, Hq*64], k, v [B*N, Hkv*64]
    -> [B*N, Hq*64].  lens [B] (optional): the scores of the keys >= lens[b] are -inf for EVERY query row of sample b, the rows
    past lens[b] included (the next layer reads them); lens[b] >= 1."""
    g = Hq // Hkv
    Q = q.to(F64).view(B, N, Hq, HEAD_DIM).transpose(1, 2)
    K = k.to(F64).view(B, N, Hkv, HEAD_DIM).transpose(1, 2).repeat_interleave(g, dim=1)
    V = v.to(F64).view(B, N, Hkv, HEAD_DIM).transpose(1, 2).repeat_interleave(g, dim=1)
    S = Q @ K.transpose(-1, -2) / math.sqrt(HEAD_DIM)
    if lens is not None:
        lens = torch.as_tensor(lens, device=S.device).view(B, 1, 1, 1)
        assert bool((lens >= 1).all())
        S = S.masked_fill(torch.arange(N, device=S.device).view(1, 1, 1, N) >= lens, float("-inf"))
    O = torch.softmax(S, -1) @ V
    return O.transpose(1, 2).reshape(B * N, Hq * HEAD_DIM)


# ---- the fused attention of one KV group ----------------------------------------------------------------------------------
def attention_group(q, k, v, rnd, inv_freq=None):
    """RoPE + softmax(q k^T / 8) v of ONE KV group from the projections as they leave the accumulator: q [B, N, G*64] (the G
    query heads that share the group), k, v [B, N, 64].  Rounded: q and k after RoPE, v, the un-normalised probabilities
    that enter PV, the output; maxima and sums stay fp64.  Returns [B, N, G*64]."""
    B, N, _ = q.shape
    G = q.shape[-1] // HEAD_DIM
    cos, sin = (c.to(q.device) for c in rope_tables(N, inv_freq))
    qg = rnd(apply_rope(q.reshape(B, N, G, HEAD_DIM), cos, sin)).transpose(1, 2)       # [B, G, N, hd]
    kg = rnd(apply_rope(k.reshape(B, N, 1, HEAD_DIM), cos, sin)).transpose(1, 2)       # [B, 1, N, hd]
    vg = rnd(v).reshape(B, N, 1, HEAD_DIM).transpose(1, 2)
    s = (qg @ kg.transpose(-1, -2)) / math.sqrt(HEAD_DIM)
    p = torch.exp(s - s.max(-1, keepdim=True).values)
    o = (rnd(p) @ vg) / p.sum(-1, keepdim=True)
    return rnd(o.transpose(1, 2).reshape(B, N, G * HEAD_DIM))


def qkv_attention_group(a, wq, wk, wv, rnd, inv_freq=None, bq=None, bk=None, bv=None, row_scale=None):
    """The fused kernel's unit of work: q/k/v projection + `attention_group`.  a [B, N, K] and wq [G*64, K], wk, wv [64, K] as
    the GEMM sees them (already rounded by the caller); optional biases and a per-row scale of the accumulator (the folded
    norms' rstd [B, N, 1], applied before the bias)."""
    def proj(w, b):
        y = a @ w.T
        if row_scale is not None:
            y = y * row_scale
        return y + b if b is not None else y
    return attention_group(proj(wq, bq), proj(wk, bk), proj(wv, bv), rnd, inv_freq)


def cfg_euler_step(x_pred_2b, z, cfg_scale, t, dt):
    """One CFG combine + Euler update on the double batch [cond; uncond] (t, dt: fp32 schedule values), in fp64"""
    B = z.shape[0]
    if cfg_scale != 1.0:
        xc, xu = x_pred_2b[:B], x_pred_2b[B:]
        x = xu + float(cfg_scale) * (xc - xu)
    else:
        x = x_pred_2b
    if t < 0.999:
        return z + (x - z) / float(np.float32(1) - np.float32(t) + np.float32(1e-5)) * float(np.float32(dt))
    return x


# ---- the model ------------------------------------------------------------------------------------------------------------
class Twin:
    """The forward of JaT_AudioSR_V3 (norm 'rms') / _V2 ('ln') on fp64 tensors, rounding through `rnd` at the stated points."""

    def __init__(self, cfg, sd, rnd=identity, norm="rms", fold=False, device="cpu"):
        self.rnd, self.norm, self.fold, self.device = rnd, norm, fold, torch.device(device)
        self.D, self.depth = cfg["hidden_size"], cfg["depth"]
        self.Hq, self.Hkv = cfg["num_q_heads"], cfg["num_kv_heads"]
        self.P, self.Cin = cfg.get("patch_len", 4), cfg.get("input_channels", 1024)
        assert self.D // self.Hq == HEAD_DIM and not (fold and norm != "rms")
        self.sd = {k: t64(v).to(self.device) for k, v in sd.items() if ".rope." not in k}
        self._w = {}

    def w(self, key):
        """a GEMM weight as the kernels hold it: rounded once"""
        if key not in self._w:
            self._w[key] = self.rnd(self.sd[key])
        return self._w[key]

    def _nw(self, key):
        return self.sd[key] if self.norm == "rms" else None

    def _planes(self, x):
        """the folded sampler keeps the residual stream as hi = rnd(x), lo = rnd(x - hi)"""
        if not self.fold:
            return x
        hi = self.rnd(x)
        return hi + self.rnd(x - hi)

    def _normed_linear(self, x, nkey, shift, scale, wkeys, bias):
        """[rnd(norm(x) (1 + scale) + shift) @ rnd(W)^T + bias for W in wkeys]; fold=True: the same function with the folded
        norms' rounding points.  shift / scale: [B, D] ([1, D] when folded) or None."""
        if not self.fold:
            xn = norm_rows(x, self._nw(nkey), self.norm)
            if scale is not None:
                xn = xn * (1 + scale[:, None, :]) + shift[:, None, :]
            a = self.rnd(xn)
            return [a @ self.w(k).T + (b if b is not None else 0.0) for k, b in zip(wkeys, bias)]
        assert scale is None or scale.shape[0] == 1, "folded weights: one modulation row per step"
        g = self.sd[nkey] * (1 + scale[0]) if scale is not None else self.sd[nkey]
        rstd = 1.0 / torch.sqrt((x * x).mean(-1, keepdim=True) + 1e-6)
        hi = self.rnd(x)
        out = []
        for k, b in zip(wkeys, bias):
            y = (hi @ self.rnd(self.sd[k] * g[None, :]).T) * rstd
            if shift is not None:
                y = y + self.rnd(shift[0]) @ self.w(k).T
            out.append(y + (b if b is not None else 0.0))
        return out

    # -- pieces ---------------------------------------------------------------------------------------------------------
    def patch_embed(self, x_in):
        """x_in [B, Cin + Cc, T] (T % P == 0) -> [B, N, D]"""
        B, C, T = x_in.shape
        P = self.P
        a = self.rnd(x_in.reshape(B, C, T // P, P).permute(0, 2, 1, 3).reshape(B, T // P, C * P))
        h = self.rnd(gelu_erf(a @ self.w("patch_embed.proj.0.weight").T + self.sd["patch_embed.proj.0.bias"]))
        return self._planes(h @ self.w("patch_embed.proj.2.weight").T + self.sd["patch_embed.proj.2.bias"])

    def t_embed(self, t):
        e = time_embedding(t, self.D)
        h = silu(e @ self.sd["t_embedder.1.weight"].T + self.sd["t_embedder.1.bias"])
        return h @ self.sd["t_embedder.3.weight"].T + self.sd["t_embedder.3.bias"]

    def adaln(self, i, t_emb):
        p = f"blocks.{i}.adaLN_modulation.1."
        return self.rnd(silu(t_emb)) @ self.w(p + "weight").T + self.sd[p + "bias"]

    def attention(self, i, qkv):
        """q, k, v [B, N, .] as the projections leave the accumulator -> rounded attention output [B, N, D]"""
        q, k, v = qkv
        g = (self.Hq // self.Hkv) * HEAD_DIM
        return torch.cat([attention_group(q[..., kv * g:(kv + 1) * g], k[..., kv * HEAD_DIM:(kv + 1) * HEAD_DIM],
                                          v[..., kv * HEAD_DIM:(kv + 1) * HEAD_DIM], self.rnd) for kv in range(self.Hkv)], -1)

    def block(self, i, x, t_emb=None, mod=None):
        """DiTBlock_GQA.forward: x [B, N, D]; t_emb [B, D], or the modulation rows mod [B or 1, 6D] themselves"""
        p = f"blocks.{i}."
        if mod is None:
            mod = self.adaln(i, t_emb)
        sh_a, sc_a, g_a, sh_m, sc_m, g_m = torch.split(mod, self.D, dim=1)
        qkv = self._normed_linear(x, p + "norm1.weight", sh_a, sc_a,
                                  [p + f"attn.{n}_proj.weight" for n in "qkv"], [None] * 3)
        ao = self.attention(i, qkv)
        x = self._planes(x + g_a[:, None, :] * (ao @ self.w(p + "attn.out_proj.weight").T))
        (h,) = self._normed_linear(x, p + "norm2.weight", sh_m, sc_m, [p + "mlp.0.weight"], [self.sd[p + "mlp.0.bias"]])
        h = self.rnd(gelu_erf(h))
        return self._planes(x + g_m[:, None, :] * (h @ self.w(p + "mlp.3.weight").T + self.sd[p + "mlp.3.bias"]))

    def final(self, x, T):
        """final norm + final linear + unpatchify: x [B, N, D] -> [B, Cin, N * P][:, :, :T]"""
        B, N, _ = x.shape
        (y,) = self._normed_linear(x, "final_layer.0.weight", None, None, ["final_layer.1.weight"], [self.sd["final_layer.1.bias"]])
        return y.reshape(B, N, self.Cin, self.P).permute(0, 2, 1, 3).reshape(B, self.Cin, N * self.P)[:, :, :T]

    def forward(self, x_t, t, x_cond, stages=None):
        x_t, t, x_cond = (t64(a).to(self.device) for a in (x_t, t, x_cond))
        T = x_t.shape[-1]
        pad = (self.P - T % self.P) % self.P
        if pad:
            x_t = torch.nn.functional.pad(x_t, (0, pad))
            x_cond = torch.nn.functional.pad(x_cond, (0, pad))
        x = self.patch_embed(torch.cat([x_t, x_cond], 1))
        if self.fold:
            assert bool((t == t[0]).all()), "folded weights: one t per step"
        t_emb = self.t_embed(t[:1] if self.fold else t)
        if stages is not None:
            stages["patch_embed"], stages["t_emb"] = x, t_emb
        for i in range(self.depth):
            x = self.block(i, x, t_emb)
            if stages is not None:
                stages[f"block{i}"] = x
        return self.final(x, T)

    __call__ = forward

    def sample(self, lr_latent, z0, num_steps, cfg_scale):
        """flow_matching_sample with the noise z0 supplied: `num_steps` CFG Euler steps, the state in fp64"""
        lr, z = t64(lr_latent).to(self.device), t64(z0).to(self.device).clone()
        B = lr.shape[0]
        ts = linspace_f32(0.0, 1.0, num_steps + 1)
        for i in range(num_steps):
            tb = torch.full((B,), float(ts[i]), dtype=F64, device=self.device)
            if cfg_scale != 1.0:
                xp = self.forward(torch.cat([z, z]), torch.cat([tb, tb]), torch.cat([lr, torch.zeros_like(lr)]))
            else:
                xp = self.forward(z, tb, lr)
            z = cfg_euler_step(xp, z, cfg_scale, ts[i], np.float32(ts[i + 1] - ts[i]))
        return z
