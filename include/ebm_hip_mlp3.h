/*
 * ebm_hip_mlp3.h -- companion of ebm_hip.h: the three-hidden-layer SiLU MLP energy, its energy kind and its two entries.  They
 * are exported by the same libebm_hip.so under the same ABI version (EBM_ABI_VERSION 9; ebm_hip.h itself is unchanged: its 58
 * entries, nothing moved) and follow every convention of ebm_hip.h: return codes, ebm_energy_t, the Philox coordinates, the
 * stream argument.  A caller of these entries includes this header, which includes ebm_hip.h.
 */
#ifndef EBM_HIP_MLP3_H
#define EBM_HIP_MLP3_H

#include "ebm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * E(x) = w4 . silu(W3 silu(W2 silu(W1 x + b1) + b2) + b3) + b4 -- the network both energy-matching examples of the reference
 * write by hand (Linear(d, H) - SiLU - Linear(H, H) - SiLU - Linear(H, H) - SiLU - Linear(H, 1)).
 *     kind = EBM_ENERGY_MLP3   n_comp = H   dev0 = the packed parameters, fp32, torch Linear layout:
 *         W1[H, dim]  b1[H]  W2[H, H]  b2[H]  W3[H, H]  b3[H]  w4[H]  b4[1]
 * Shapes: H = 64 with 1 <= dim <= 128 (split-bf16 images of all three matrices resident in LDS, bf16 matrix pipe at fp32
 * accuracy), or H = 128 with 1 <= dim <= 32 (fp32 weights resident in LDS, exact-f32 matrix instruction); anything else is
 * EBM_EDIM.  The kind is a value of ebm_energy_t.kind that only the two entries below take: every entry of ebm_hip.h and of
 * its other companions refuses it with EBM_EKIND.
 */
#define EBM_ENERGY_MLP3 8

/*
 * E(x) and dE/dx at n_chains points in ONE launch.  x [n_chains, dim]; energy_out [n_chains] or NULL; grad_out
 * [n_chains, dim] or NULL (NULL: the forward pass only).  x and grad_out 16-byte aligned.
 * Refusals, in this order and before any device access: a NULL energy (EBM_EINVAL); a kind other than EBM_ENERGY_MLP3
 * (EBM_EKIND); NULL dev0 or x, n_chains < 0 (EBM_EINVAL); the shape table (EBM_EDIM); alignment (EBM_EINVAL).  n_chains == 0,
 * or both outputs NULL, returns 0 without a launch.
 */
EBM_API int ebm_energy_grad_mlp3_f32(const ebm_energy_t* energy, const float* x, int64_t n_chains, int32_t dim,
                                     float* energy_out, float* grad_out, void* stream);

/*
 * k_steps Euler-Maruyama Langevin steps on the energy in ONE launch, out of place like ebm_langevin_chain_from_f32: the chains
 * start from x_src [n_chains, dim] and the final state is written to x [n_chains, dim]; x_src == x is the in-place call, any
 * other overlap is EBM_EINVAL.  Step i = 0 .. k_steps - 1, every multiply and add rounded on its own (the reference's order):
 *     g  = dE/dx(x)
 *     x1 = x - eta * g
 *     x  = x1 + noise_coef * (z_i * sqrt_eta)
 * z_i: noise[i] of the caller's [k_steps, n_chains, dim] field, or (noise == NULL) the library's Philox normal field of (seed)
 * at step offset + i, element chain * dim + column -- what ebm_noise_fill_f32(EBM_NOISE_NORMAL) writes for n_chains * dim
 * elements at that step, so a native call equals the injected call on the materialised field bit for bit, and a call of k
 * steps equals two calls of k1 + k2 = k steps with the offset advanced by k1.
 * Rows at and beyond n_chains of an over-allocated x are not touched; x_src is only read.
 * Refusals as at ebm_energy_grad_mlp3_f32, with k_steps < 0 among the EBM_EINVAL ones.  n_chains == 0 returns 0 without a
 * launch; k_steps == 0 copies x_src to x (nothing when they are the same) without a launch.
 */
EBM_API int ebm_langevin_chain_mlp3_f32(const ebm_energy_t* energy, const float* x_src, float* x, int64_t n_chains,
                                        int32_t dim, int32_t k_steps, float eta, float sqrt_eta, float noise_coef,
                                        const float* noise, uint64_t seed, uint64_t offset, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EBM_HIP_MLP3_H */
