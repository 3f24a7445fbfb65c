// CFG combine + Euler step of the sampler (infer_test_v3m2.py:161-179), per element: the ONE definition used by
// cfg_euler_kernel (elementwise.hip) and by the final Linear's EPI_CFG_EULER epilogue (gemm.hip).
//   x = u + s (c - u);   z' = z + (x - z) / denom * dt   (t < 0.999)   |   z' = x   (otherwise: `direct`)
// The multiply-adds are spelled out as the fused forms the compiler chose for cfg_euler_kernel, so that both kernels round
// alike whatever -ffp-contract makes of the code around them.
//
// Two-stage solvers (midpoint, Heun: DESIGN.md 15) reuse the Euler formula for their first stage (step length c, the old latent
// kept as z_base) and finish with the general second stage
//   z' = a z_base + b z + c (x - z) / denom
// cfg_stage_kernel (elementwise.hip) and the EPI_CFG_STAGE epilogue (gemm.hip) both call jat_stage_step: five fp32 roundings
// (x - z; the quotient; b z; the fused a z_base + .; the fused . c + .) after the two of the CFG combine.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ float jat_cfg_combine(float c, float u, float s) { return __builtin_fmaf(s, c - u, u); }
__device__ __forceinline__ float jat_euler_step(float x, float z, float denom, float dt) {
  return __builtin_fmaf(__fdiv_rn(x - z, denom), dt, z);
}
__device__ __forceinline__ float jat_stage_step(float x, float z, float z_base, float denom, float a, float b, float c) {
  return __builtin_fmaf(__fdiv_rn(x - z, denom), c, __builtin_fmaf(a, z_base, __fmul_rn(b, z)));
}
