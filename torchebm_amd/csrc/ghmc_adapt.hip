// Generalized HMC with per-chain dual-averaging step-size adaptation (ebm_ghmc_adapt_chain_f32): the refusals the adaptation
// adds, geometry and dispatch to the per-energy units (ghmc_adapt_unit.hip, one object per kind; the kernel: ghmc_adapt_kernel.h).
#include <cmath>

#include "ghmc_adapt_kernel.h"
#include "ghmc_adapt_launch.h"

namespace ebm {

int ghmc_adapt_check(const GhmcAdaptChainReq& q, const char* who) {
  if (!q.da) return fail(EBM_EINVAL, "%s: da pointer is NULL", who);
  if (q.n_adapt < 0 || q.n_adapt > q.n_mh)
    return fail(EBM_EINVAL, "%s: n_adapt=%d outside 0 .. n_mh=%d", who, q.n_adapt, q.n_mh);
  if (q.n_adapt > 0 && !q.da_table) return fail(EBM_EINVAL, "%s: da_table pointer is NULL with n_adapt=%d", who, q.n_adapt);
  if (q.init_da < 0 || q.init_da > (EBM_DA_INIT | EBM_DA_OPEN)) return fail(EBM_EINVAL, "%s: init_da=%d (bits 0 .. 1)", who, q.init_da);
  if (!(q.target_accept > 0.0 && q.target_accept < 1.0))
    return fail(EBM_EINVAL, "%s: target_accept=%g (must lie in (0, 1))", who, q.target_accept);
  if (!(q.eps0 > 0.0) || !(q.eps_min > 0.0) || !(q.eps_max > 0.0) || !std::isfinite(q.eps0) || !std::isfinite(q.eps_min) ||
      !std::isfinite(q.eps_max) || q.eps_min > q.eps_max)
    return fail(EBM_EINVAL, "%s: eps0=%g eps_min=%g eps_max=%g (all must be positive and finite, eps_min <= eps_max)", who, q.eps0,
                q.eps_min, q.eps_max);
  if (!std::isfinite(q.mu)) return fail(EBM_EINVAL, "%s: mu=%g (must be finite)", who, q.mu);
  return 0;
}

int ghmc_adapt_chain_launch(const GhmcAdaptChainReq& q, hipStream_t st) {
  using namespace rows;
  const char* who = "ebm_ghmc_adapt_chain_f32";
  if (int r = ghmc_check_geometry(q.dim)) return r;
  Geometry geo;
  pick_geometry(q.dim, geo);
  ghmc_adapt::GhmcAdaptArgs a{};
  a.x = q.x; a.v = q.v; a.n_chains = q.n_chains; a.dim = q.dim; a.n_mh = q.n_mh; a.n_leapfrog = q.n_leapfrog;
  a.thin = q.thin; a.n_kept = q.n_kept(); a.draw_v0 = q.draw_v0 ? 1 : 0;
  a.n_adapt = q.n_adapt; a.init_da = (q.init_da & EBM_DA_INIT) ? 1 : 0; a.keep_open = (q.init_da & EBM_DA_OPEN) ? 1 : 0;
  // every double rounded once; gamma L and the two logs formed in double
  a.full_refresh = std::isinf(q.gamma) ? 1 : 0;
  a.eps0 = (float)q.eps0;
  a.gamma_l = a.full_refresh ? 0.0f : (float)(q.gamma * (double)q.n_leapfrog);
  a.temp = (float)q.temperature; a.sqrt_temp = (float)sqrt(q.temperature); a.beta = (float)(1.0 / q.temperature);
  a.delta = (float)q.target_accept; a.mu = (float)q.mu;
  a.log_eps_min = (float)log(q.eps_min); a.log_eps_max = (float)log(q.eps_max);
  a.da = q.da; a.da_table = q.da_table; a.eps_trace = q.eps_trace; a.alpha_mean = q.alpha_mean;
  a.traj = q.traj; a.accept_mask = q.accept_mask; a.noise = q.noise; a.u = q.u;
  a.key = q.key(); a.step0 = q.offset;
  size_t smem = 0;
  plan_params(q.e, q.dim, geo, a.energy, a.param_floats, smem);
  const int64_t blocks = blocks_for(q.n_chains, geo);
  if (blocks > 0x7fffffffLL) return fail(EBM_EINVAL, "%s: too many chains for one launch", who);
  const dim3 grid((unsigned)blocks);
  for_kind(q.e.kind, [&](auto K) { ghmc_adapt::launch_kind<decltype(K)::value>(geo, grid, smem, st, a); });
  return check_launch(who);
}

}  // namespace ebm
