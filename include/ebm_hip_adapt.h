/*
 * ebm_hip_adapt.h -- companion of ebm_hip.h: the entry that runs generalized HMC (and, with gamma = +inf, plain HMC) while every
 * chain adapts its own leapfrog step size by Nesterov dual averaging towards a target acceptance (Hoffman & Gelman 2014,
 * section 3.2), in ONE launch.  It is exported by the same libebm_hip.so under the same ABI version (EBM_ABI_VERSION 9;
 * ebm_hip.h itself is unchanged: its 58 entries, nothing moved) and follows every convention of ebm_hip.h: return codes,
 * ebm_energy_t, the Philox coordinates, the stream argument.  A caller of this entry includes this header, which includes
 * ebm_hip.h.
 */
#ifndef EBM_HIP_ADAPT_H
#define EBM_HIP_ADAPT_H

#include "ebm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the bits of `init_da` */
#define EBM_DA_INIT 1 /* da is output only: every chain starts from (fp32(eps0), 0, 0) */
#define EBM_DA_OPEN 2 /* the call does not close the adaptation (below): a later call continues it */

/*
 * ebm_ghmc_chain_f32's parameter list with `eps` replaced by the eleven parameters from `eps0` to `alpha_mean`.  The walk is that
 * entry's, draw for draw: the lane geometry (dim <= 256, every analytic kind), the kinetic energy, the pseudo-transition that
 * evaluates the start state, the carried energy and force, the safe-mode leapfrog trajectory, the flip, traj / thin,
 * accept_mask, the injected noise / u, draw_v0, the Philox coordinates (v0 at step offset, the normals of transition t at
 * offset + 1 + 2 t, its uniform at offset + 2 + 2 t) and the steps a call owns (2 n_mh + 1).  What differs: the step size is a
 * value of the chain.  Nothing is reduced across chains -- no exchange, no barrier, no atomic; a caller that wants ONE step size
 * pools da row 0 afterwards.
 *
 * Doubles are rounded once to fp32 in the entry: eps0, target_accept (delta), mu, temperature (T), sqrt(T), 1 / T (beta),
 * gamma * n_leapfrog (the product formed in double), log(eps_min) and log(eps_max) (the logs formed in double).
 *
 * da        [3, n_chains], in and out: row 0 the step size the chain's next transition uses, row 1 H-bar, row 2 log eps-bar.
 *           With EBM_DA_INIT set it is output only and every chain starts from (fp32(eps0), 0, 0).
 * da_table  device [n_adapt, 5], supplied by the caller: row t = (1 - w, w, s, k, 1 - k) with m = m0 + t + 1,
 *           w = 1 / (m + t0), s = sqrt(m) / gamma_da, k = m^(-kappa); each value formed in double and rounded once.  m0 is
 *           the number of adapting transitions earlier calls made (0 for a fresh start); t0, gamma_da, kappa are the
 *           dual-averaging constants (Stan: 10, 0.05, 0.75).
 * n_adapt   the first n_adapt transitions adapt, 0 <= n_adapt <= n_mh; later ones run frozen at da row 0.
 * eps_trace [n_mh, n_chains] or NULL: the step size transition t ran at.
 * alpha_mean [n_chains] or NULL: the mean of alpha over the adapting transitions, 0 when n_adapt == 0.
 *
 * Transition t of a chain, every product and sum rounded on its own (tab = da_table):
 *     eps = da0
 *     gamma finite:  span = fp32(gamma L) * eps;  c1 = expf(-span);  c2 = sqrtf(fp32(T) * (-expm1f(-2 * span)))
 *     gamma = +inf:  c1 = 0, c2 = sqrt_temp
 *     O step, u, H0, the trajectory at (eps, 0.5f * eps), H1, the decision, the flip:  as ebm_ghmc_chain_f32
 *     alpha = min(1, exp(clamp(beta * (H0 - H1), +-50)));  NaN counts as 0     (the value the decision already forms)
 *     if t < n_adapt:
 *         Hbar  = tab[t][0] * Hbar + tab[t][1] * (delta - alpha)
 *         le    = clamp(mu - tab[t][2] * Hbar, log eps_min, log eps_max)
 *         lbar  = tab[t][3] * le + tab[t][4] * lbar
 *         da0   = (t + 1 == n_adapt and EBM_DA_OPEN is not set) ? expf(lbar) : expf(le)        (the close)
 * The three values are stored once, at the end, with x and v.
 *
 * Consequences:
 *   - The close replaces the last iterate exp(le) by the averaged one exp(lbar), so a call that closes cannot be continued
 *     into the bits of a longer adapting call: the iterate is gone.  A call with EBM_DA_OPEN keeps it.  With n_adapt == n_mh in
 *     both calls, (n1, table m0 = 0, EBM_DA_INIT | EBM_DA_OPEN) followed by (n2, table m0 = n1, init_da = 0, offset + 2 n1,
 *     draw_v0 = 0) gives the bits of one call of n1 + n2 -- x, v, da, traj, accept_mask, eps_trace.
 *   - A closed call (n1 = n_adapt) followed by a frozen one (n_adapt = 0, init_da = 0) gives the bits of one call of n_mh =
 *     n1 + n2 with n_adapt = n1.
 *   - n_adapt == 0, gamma = +inf, da row 0 == eps in every chain: x, v, traj and accept_mask are ebm_ghmc_chain_f32's at
 *     that eps bit for bit.
 *
 * Refusals: ebm_ghmc_chain_f32's, in its order (eps0 in the place of eps).  Further EBM_EINVAL, behind them and in front of
 * any device access and of the early return for n_chains == 0, no buffer touched: a NULL da; n_adapt outside 0 .. n_mh; a NULL
 * da_table with n_adapt > 0; init_da outside 0 .. 3; target_accept not in (0, 1); eps0, eps_min or eps_max not positive and
 * finite, or eps_min > eps_max; mu not finite.
 */
EBM_API int ebm_ghmc_adapt_chain_f32(const ebm_energy_t* energy, float* x, float* v, int64_t n_chains, int32_t dim,
                                     int32_t n_mh, int32_t n_leapfrog, double eps0, double target_accept, double mu,
                                     double eps_min, double eps_max, int32_t n_adapt, int32_t init_da, float* da,
                                     const float* da_table, float* eps_trace, float* alpha_mean, double gamma,
                                     double temperature, int32_t draw_v0, int32_t thin, float* traj, uint8_t* accept_mask,
                                     const float* noise, const float* u, uint64_t seed, uint64_t offset, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EBM_HIP_ADAPT_H */
