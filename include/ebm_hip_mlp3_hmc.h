/*
 * ebm_hip_mlp3_hmc.h -- companion of ebm_hip_mlp3.h: the HMC transition kernel of the three-hidden-layer SiLU MLP energy at
 * hidden width 64.  Exported by the same libebm_hip.so under the same ABI version (EBM_ABI_VERSION 9; ebm_hip.h and
 * ebm_hip_mlp3.h are unchanged) and following every convention of ebm_hip.h: return codes, ebm_energy_t, the Philox
 * coordinates, the mass kinds, the stream argument.  A caller of this entry includes this header, which includes the others.
 */
#ifndef EBM_HIP_MLP3_HMC_H
#define EBM_HIP_MLP3_HMC_H

#include "ebm_hip_mlp3.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * n_mh Metropolis-corrected HMC transitions of n_leapfrog leapfrog steps on an EBM_ENERGY_MLP3 energy (ebm_hip_mlp3.h:
 * n_comp = 64, dev0 = the packed parameters), 1 <= dim <= 128, in ONE launch, with the semantics ebm_hip.h documents for
 * ebm_hmc_chain_f32 (safe mode: force clamp at +-1e6, nan_to_num on x and p, H = clamp(E, +-1e10) + clamp(K, 0, 1e10),
 * accept iff u < min(1, exp(clamp(H0 - H1, +-50))), a NaN rejects), L + 1 evaluations per transition.
 *   x             [n_chains, dim] in/out; rows at and beyond n_chains of an over-allocated x are not touched
 *   eps_table     device [n_mh] or NULL: the step size of transition t (NULL: eps)
 *   mass_kind     EBM_MASS_NONE or EBM_MASS_SCALAR (mass_scalar = m: p ~ sqrt(m) z, K = 0.5 p.p / m, drift eps / max(m, 1e-10)).
 *                 m is not checked, as in ebm_hmc_chain_f32: m = 0 makes K infinite or NaN and m < 0 makes every momentum NaN
 *                 (sqrt of a negative number), so every proposal is rejected and x is left as it was.
 *   traj          [n_chains, n_mh / thin, dim] or NULL: the held state behind every thin-th transition
 *   accept_mask   [n_mh, n_chains] or NULL, filled;   accept_count [n_mh] or NULL, ADDED to
 *   p_noise, u    the caller's [n_mh, n_chains, dim] normals and [n_mh, n_chains] uniforms, or NULL: the library's Philox
 *                 fields of (seed) -- momenta of transition t at step offset + 2 t, element chain * dim + column; the uniform at
 *                 step offset + 2 t + 1, element chain -- what ebm_noise_fill_f32 writes there, so a native call equals the
 *                 injected call on the materialised fields bit for bit, and a call of n transitions equals two calls of
 *                 n1 + n2 = n with the offset advanced by 2 n1.
 * Refusals, in this order, before any device access and before the early return: a NULL energy (EBM_EINVAL); a kind other
 * than EBM_ENERGY_MLP3 (EBM_EKIND); NULL dev0 or x, n_chains < 0, n_mh < 0, n_leapfrog < 1, thin < 1 (EBM_EINVAL); hidden
 * width other than 64 or dim outside 1 .. 128 (EBM_EDIM); a mass kind other than none / scalar (EBM_EINVAL); x, traj or
 * p_noise not 16-byte aligned (EBM_EINVAL).  n_chains == 0 or n_mh == 0 returns 0 without a launch.
 */
EBM_API int ebm_hmc_chain_mlp3_f32(const ebm_energy_t* energy, float* x, int64_t n_chains, int32_t dim, int32_t n_mh,
                                   int32_t n_leapfrog, float eps, const float* eps_table, int32_t mass_kind,
                                   double mass_scalar, int32_t thin, float* traj, uint8_t* accept_mask,
                                   uint32_t* accept_count, const float* p_noise, const float* u, uint64_t seed,
                                   uint64_t offset, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EBM_HIP_MLP3_HMC_H */
