/*
 * ebm_hip_adapt_mass.h -- companion of ebm_hip_adapt.h: the entry that adapts every chain's leapfrog step size by dual averaging
 * (ebm_ghmc_adapt_chain_f32) while the walk carries a scalar or diagonal mass (ebm_ghmc_chain_mass_f32), in ONE launch.  It is
 * exported by the same libebm_hip.so under the same ABI version (EBM_ABI_VERSION 9; ebm_hip.h and ebm_hip_adapt.h are unchanged)
 * and follows every convention of ebm_hip.h.  A caller of this entry includes this header, which includes ebm_hip_adapt.h.
 */
#ifndef EBM_HIP_ADAPT_MASS_H
#define EBM_HIP_ADAPT_MASS_H

#include "ebm_hip_adapt.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ebm_ghmc_adapt_chain_f32's parameter list with `int32_t mass_kind, double mass_scalar, const float* mass_diag` directly behind
 * `temperature`, where the massed entries of ebm_hip.h put them.
 *
 * The walk is ebm_ghmc_adapt_chain_f32's, draw for draw: the same Philox coordinates (the start draw at step offset, the normals
 * of transition t at offset + 1 + 2 t, its uniform at offset + 2 + 2 t), a call owns 2 n_mh + 1 steps; draw_v0, traj / thin,
 * accept_mask, the injected noise / u, the controller recurrence and da_table, the close and EBM_DA_OPEN, eps_trace, alpha_mean,
 * the pseudo-transition t = -1 and "NaN alpha counts as 0" are unchanged (ebm_hip_adapt.h).
 *
 * The mass forms are those of ebm_ghmc_chain_mass_f32 (ebm_hip.h), formed exactly as there: EBM_MASS_SCALAR forms m_raw = fp32(m),
 * m_sqrt = fp32(sqrt(m)), m_safe = fp32(max(m, 1e-10)) in double, each rounded once; EBM_MASS_DIAG reads m_raw_j = mass_diag[j]
 * (device, [dim]; never written) and forms m_sqrt_j = sqrtf(m_raw_j), correctly rounded, and m_safe_j = max(m_raw_j, 1e-10f).
 * The carried plane `v` is the MOMENTUM p ~ N(0, T m); with draw_v0, p = (sqrt_temp * m_sqrt_j) * z0.
 *
 * Transition t of a chain with this chain's eps = da0, every operation rounded on its own:
 *     gamma finite:  span = fp32(gamma L) * eps;  c1 = expf(-span);  c2 = sqrtf(fp32(T) * (-expm1f(-2 * span)))
 *     gamma = +inf:  c1 = 0, c2 = sqrt_temp
 *     refresh_j = c2 * m_sqrt_j;   p = c1 * p + refresh_j * z
 *     drift_j   = eps / m_safe_j                                         (an IEEE division)
 *     H = clamp(E, +-1e10) + K_m(p),  K_m(p) = clamp(0.5 sum_j p_j^2 / m_raw_j, 0, 1e10)   (scalar: (0.5 sum_j p_j^2) / m_raw)
 *     the trajectory of ebm_ghmc_chain_mass_f32 at (drift, eps, 0.5f * eps): x += drift_j p_j, the kicks with eps
 *     accept on beta * (H0 - H1); alpha is the value the decision forms; a reject hands back -(p after O)
 *     the controller update:  as ebm_hip_adapt.h
 *
 * Identities, bit for bit:
 *   a. mass_scalar == 1.0, or a diagonal of ones: x, v, da, traj, accept_mask, eps_trace and alpha_mean are
 *      ebm_ghmc_adapt_chain_f32's.
 *   b. n_adapt == 0, gamma = +inf, da row 0 == eps in every chain: x, p, traj and accept_mask are ebm_ghmc_chain_mass_f32's at
 *      that eps and the same mass (with T = 1: ebm_hmc_chain_f32's x and mask with that mass).
 *   c. Both "two calls equal one" forms of ebm_hip_adapt.h hold with a mass.
 *
 * Refusals: ebm_ghmc_adapt_chain_f32's, in its order; then EBM_EINVAL for mass_kind == EBM_MASS_NONE or an unknown kind, a NULL
 * mass_diag with EBM_MASS_DIAG, a mass_scalar that is not positive and finite (with EBM_MASS_SCALAR).  All stand in front of any
 * device access and of the early return for n_chains == 0; a refused call touches no buffer.  The MLP energy is refused with
 * EBM_EKIND.
 */
EBM_API int ebm_ghmc_adapt_chain_mass_f32(const ebm_energy_t* energy, float* x, float* v, int64_t n_chains, int32_t dim,
                                          int32_t n_mh, int32_t n_leapfrog, double eps0, double target_accept, double mu,
                                          double eps_min, double eps_max, int32_t n_adapt, int32_t init_da, float* da,
                                          const float* da_table, float* eps_trace, float* alpha_mean, double gamma,
                                          double temperature, int32_t mass_kind, double mass_scalar, const float* mass_diag,
                                          int32_t draw_v0, int32_t thin, float* traj, uint8_t* accept_mask, const float* noise,
                                          const float* u, uint64_t seed, uint64_t offset, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EBM_HIP_ADAPT_MASS_H */
