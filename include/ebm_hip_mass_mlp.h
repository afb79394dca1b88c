/*
 * ebm_hip_mass_mlp.h -- companion of ebm_hip.h: the two entries that run underdamped Langevin (BAOAB) and generalized HMC with
 * a scalar or diagonal mass on the MLP energy, each in ONE launch.  They are exported by the same libebm_hip.so under the same
 * ABI version (EBM_ABI_VERSION 9; ebm_hip.h itself is unchanged: its 58 entries, nothing moved) and follow every convention
 * of ebm_hip.h: return codes, ebm_energy_t, EBM_MASS_*, the Philox coordinates, the stream argument.  A caller of these two
 * entries includes this header, which includes ebm_hip.h.
 */
#ifndef EBM_HIP_MASS_MLP_H
#define EBM_HIP_MASS_MLP_H

#include "ebm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Underdamped Langevin (BAOAB) with a scalar or diagonal mass on the MLP energy, in ONE launch (an addition to ABI 9: nothing
 * else moved): ebm_kinetic_mlp_chain_f32's parameter list with `int32_t mass_kind, double mass_scalar, const float* mass_diag`
 * directly behind `temperature`, as ebm_kinetic_chain_mass_f32 extends ebm_kinetic_chain_f32's.  ebm_ghmc_mlp_chain_mass_f32
 * (below) extends that entry's list in the same way.  The rules both share are those stated at
 * ebm_kinetic_chain_mass_f32, restated for the MLP walks:
 *
 * Mass forms: m_raw, m_sqrt, m_safe as there (the scalar forms built in double and rounded once; the diagonal's m_sqrt a
 * correctly rounded sqrtf, m_safe = m < 1e-10 ? 1e-10 : m; the entries are not inspected).  Every column at or beyond dim gets
 * mass 1; x and p stay 0 there.  Carried plane: the MOMENTUM p with law N(0, T m); `v` is that plane, in and out.  draw_v0 != 0:
 * p = (sqrt_temp * m_sqrt_j) * z0, z0 the normal field at step offset.
 *
 * Unchanged from the unit-mass MLP entries: the constants formed in double, the Philox coordinates and the steps a call owns,
 * thin / traj / accept_mask, the injected noise / u, the outputs, "two calls equal one", the shape rule (hidden width 64 / 128,
 * 1 <= dim <= 128: EBM_EDIM), the 16-byte alignment of x, v, traj and noise, every refusal and their order.  A kind other than
 * EBM_ENERGY_MLP is EBM_EKIND (the analytic kinds: ebm_kinetic_chain_mass_f32 / ebm_ghmc_chain_mass_f32).  More EBM_EINVAL,
 * behind the walk's own parameter checks and the shape rule, in front of any device access and of the early return for
 * n_chains == 0, no buffer touched: mass_kind == EBM_MASS_NONE or unknown (callers use the unit-mass entry); EBM_MASS_DIAG with
 * a NULL mass_diag; EBM_MASS_SCALAR with a mass_scalar that is not positive and finite.
 *
 * BAOAB with a mass, in the one-evaluation-site loop of ebm_kinetic_mlp_chain_f32.  a_j = hh / m_safe_j and s_j = c2 * m_sqrt_j
 * are formed once per column; evaluations i = 0 .. k_steps, every product and sum rounded on its own, g raw and unclamped:
 *     g = dE/dx(x)
 *     if i > 0:  p = p - hh * g             (the closing B of step i - 1; then x goes to traj if i % thin == 0)
 *     if i == k_steps: stop
 *     p = p - hh * g                        (the opening B: never merged with the closing one)
 *     x = x + a_j * p                       (A)
 *     p = c1 * p + s_j * z_i                (O)
 *     x = x + a_j * p                       (A)
 * With mass_scalar = 1, or a diagonal of ones, every factor is exact and x, v and traj are ebm_kinetic_mlp_chain_f32's bit for
 * bit.
 */
EBM_API int ebm_kinetic_mlp_chain_mass_f32(const ebm_energy_t* energy, float* x, float* v, int64_t n_chains, int32_t dim,
                                           int32_t k_steps, double h, double gamma, double temperature, int32_t mass_kind,
                                           double mass_scalar, const float* mass_diag, int32_t draw_v0, int32_t thin,
                                           float* traj, const float* noise, uint64_t seed, uint64_t offset, void* stream);

/*
 * Generalized HMC with a scalar or diagonal mass on the MLP energy, in ONE launch (an addition to ABI 9: nothing else moved).
 * The parameter list, the mass forms, the carried momentum plane, what stays as in ebm_ghmc_mlp_chain_f32 and the refusals:
 * the rules stated at ebm_kinetic_mlp_chain_mass_f32.  s_j = c2 * m_sqrt_j and the drift scale eps / m_safe_j are formed once
 * per column.  Transition t = 0 .. n_mh - 1, the transition of ebm_ghmc_mlp_chain_f32 with
 *     p  = c1 * p + s_j * z_t                      (O)  two products and a sum, each rounded on its own; p is stored back
 *     H  = clamp(E, +-1e10) + K_m(p),  K_m the massed kinetic energy of ebm_hmc_chain_f32: 0.5 sum(p^2 / m_raw) for a diagonal
 *          mass, (0.5 sum p^2) / m_raw for a scalar one, clamped to [0, 1e10], summed in the unit-mass entry's order
 *     the drift  x' = fma(eps / m_safe_j, p, x')   in every leapfrog step; the half kicks p = fma(eps / 2, f, p), the force
 *          clamp, the scrubs and the literal re-evaluation are untouched
 *     accepted iff u < min(1, exp(clamp(beta * (H0 - H1), +-50)));  a reject hands back -(the stored p after O)
 * With mass_scalar = 1, or a diagonal of ones, x, v, traj and accept_mask are ebm_ghmc_mlp_chain_f32's bit for bit.
 */
EBM_API int ebm_ghmc_mlp_chain_mass_f32(const ebm_energy_t* energy, float* x, float* v, int64_t n_chains, int32_t dim,
                                        int32_t n_mh, int32_t n_leapfrog, double eps, double gamma, double temperature,
                                        int32_t mass_kind, double mass_scalar, const float* mass_diag, int32_t draw_v0,
                                        int32_t thin, float* traj, uint8_t* accept_mask, const float* noise, const float* u,
                                        uint64_t seed, uint64_t offset, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EBM_HIP_MASS_MLP_H */
