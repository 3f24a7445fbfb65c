// The training loss (jat_internal.h): its checks, its plan and its one launch, for the trainer's step and the per-kernel entry points
#include <cmath>

#include "jat_internal.h"

int check_band_ratios(const LossSpec& l) {
  const bool ok = l.phase_ratio >= 0 && l.phase_ratio <= 1 && l.strict_cut >= 0 && l.soft_cut >= l.strict_cut && l.soft_cut <= 1;
  return ok ? JAT_OK : fail(JAT_E_INVALID, "band ratios must satisfy 0 <= strict <= soft <= 1 and 0 <= phase ratio <= 1");
}

int check_recon_eps(const LossSpec& l) {
  const bool ok = l.recon_eps >= 0.0 && std::isfinite(l.recon_eps) && !(l.recon_eps > 0.0 && (float)l.recon_eps == 0.f);
  return ok ? JAT_OK : fail(JAT_E_INVALID, "recon_eps must be finite and >= 0 (0 selects the MSE loss) and, if positive, not below fp32's range");
}

int check_loss_weights(const LossSpec& l) {
  const bool ok = std::isfinite(l.rw) && std::isfinite(l.lw) && std::isfinite(l.fw) && std::isfinite(l.mw) && std::isfinite(l.cw);
  return ok ? JAT_OK : fail(JAT_E_INVALID, "loss weights must be finite");
}

LossLaunch plan_loss(const LossSpec& l, int64_t rows, int T) {
  // band edges exactly as the reference computes them: int(freq_bins * ratio) in double
  auto edge = [F = T / 2 + 1](double ratio) { return (int)((double)F * ratio); };
  const size_t tw_bytes = align_up((size_t)T * sizeof(float2), 256);
  return {l.has_latent(), edge(l.phase_ratio), edge(l.strict_cut), edge(l.soft_cut), plan_latent_loss(T),
          ((size_t)train_red_blocks() + 2) * 4, tw_bytes, tw_bytes + (size_t)rows * 8 * 4};
}

std::vector<float2> make_twiddles(int T) {
  std::vector<float2> tw(T);
  for (int i = 0; i < T; ++i) {
    const double th = 2.0 * M_PI * (double)i / (double)T;
    tw[i] = float2{(float)cos(th), (float)sin(th)};
  }
  return tw;
}

int run_loss(const LossSpec& l, const LossLaunch& p, const float* pred, const float* target, const float* lr, const float2* tw,
             float* dpred, float* part, float* out, int64_t rows, int T, float loss_scale, hipStream_t s) {
  if (p.latent)
    KCHK(launch_latent_loss(pred, target, lr, tw, dpred, part, out, (int)rows, T, (float)l.lw, (float)l.fw, (float)l.mw, (float)l.cw,
                            p.low, p.strict, p.soft, (float)l.recon_eps, (float)l.rw, loss_scale, s));
  else
    KCHK(launch_recon_grad(pred, target, dpred, part, out, rows * T, l.recon_eps, loss_scale, (float)l.rw, s));
  return JAT_OK;
}
