/*
 * ebm_hip_mlp3_kinetic.h -- companion of ebm_hip_mlp3.h: underdamped (kinetic) Langevin dynamics, BAOAB, on the
 * three-hidden-layer SiLU MLP energy at hidden width 64.  Exported by the same libebm_hip.so under the same ABI version
 * (EBM_ABI_VERSION 9; ebm_hip.h and ebm_hip_mlp3.h are unchanged) and following every convention of ebm_hip.h: return codes,
 * ebm_energy_t, the Philox coordinates, the stream argument.  A caller of this entry includes this header, which includes the
 * others.
 */
#ifndef EBM_HIP_MLP3_KINETIC_H
#define EBM_HIP_MLP3_KINETIC_H

#include "ebm_hip_mlp3.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * k_steps BAOAB steps of size h (unit mass, friction gamma, temperature T) on an EBM_ENERGY_MLP3 energy (ebm_hip_mlp3.h:
 * n_comp = 64, dev0 = the packed parameters), 1 <= dim <= 128, in ONE launch of k_steps + 1 evaluations, with the parameter list
 * and the recurrence of ebm_kinetic_mlp_chain_f32 (ebm_hip.h).  With hh = (float)(h / 2), c1 = (float)exp(-gamma h),
 * c2 = (float)sqrt(T (1 - exp(-2 gamma h))) and sqrt_temp = (float)sqrt(T), each formed in double and rounded once:
 *     g = dE/dx(x)                         evaluation i = 0 .. k_steps
 *     if i > 0:  v = v - hh g              the closing kick of step i - 1; then x goes to traj if i % thin == 0
 *     if i == k_steps: stop
 *     v = v - hh g                         the opening kick, never merged with the closing one
 *     x = x + hh v
 *     v = c1 v + c2 xi_i
 *     x = x + hh v
 * every product and sum rounded on its own, the gradient raw (no clamp: a NaN stays in its chain).
 *   x        [n_chains, dim] in/out; rows at and beyond n_chains of an over-allocated x, v or traj are not touched
 *   v        [n_chains, dim]: draw_v0 == 0 in/out; draw_v0 != 0 output only, the start is sqrt_temp xi of Philox step `offset`
 *   traj     [n_chains, k_steps / thin, dim] or NULL: the position behind every thin-th step
 *   noise    the caller's [k_steps, n_chains, dim] normals, or NULL: the library's normal field of (seed) at step
 *            offset + 1 + i, element chain * dim + column -- what ebm_noise_fill_f32 writes there, so a native call equals the
 *            injected call on the materialised fields bit for bit, and with draw_v0 == 0 two calls (k1, offset) then
 *            (k2, offset + k1) equal one call of k1 + k2 bit for bit.
 * Refusals, in this order, before any device access and before the early return: a NULL energy (EBM_EINVAL); a kind other than
 * EBM_ENERGY_MLP3 (EBM_EKIND); NULL dev0, x or v, n_chains < 0, k_steps < 1, thin < 1 (EBM_EINVAL); hidden width other than 64
 * or dim outside 1 .. 128 (EBM_EDIM); h, gamma or temperature not positive and finite (EBM_EINVAL); x, v, traj or noise not
 * 16-byte aligned (EBM_EINVAL).  n_chains == 0 returns 0 without a launch.
 */
EBM_API int ebm_kinetic_chain_mlp3_f32(const ebm_energy_t* energy, float* x, float* v, int64_t n_chains, int32_t dim,
                                       int32_t k_steps, double h, double gamma, double temperature, int32_t draw_v0,
                                       int32_t thin, float* traj, const float* noise, uint64_t seed, uint64_t offset, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EBM_HIP_MLP3_KINETIC_H */
