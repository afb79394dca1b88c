// Generalized HMC with a mass and per-chain dual-averaging step-size adaptation (ebm_ghmc_adapt_chain_mass_f32): geometry and
// dispatch to the per-energy units (ghmc_adapt_mass_unit.hip, one object per kind; the kernel: ghmc_adapt_mass_kernel.h).  The
// adaptation's refusals are ghmc_adapt.hip's (ghmc_adapt_check), the geometry refusal ghmc.hip's.
#include <cmath>

#include "ghmc_adapt_mass_kernel.h"
#include "ghmc_adapt_mass_launch.h"

namespace ebm {

int ghmc_adapt_mass_chain_launch(const GhmcAdaptMassChainReq& m, hipStream_t st) {
  using namespace rows;
  const char* who = "ebm_ghmc_adapt_chain_mass_f32";
  const GhmcAdaptChainReq& q = m.chain;
  if (int r = ghmc_check_geometry(q.dim)) return r;
  Geometry geo;
  pick_geometry(q.dim, geo);
  ghmc_adapt_mass::GhmcAdaptMassArgs a{};
  a.x = q.x; a.v = q.v; a.n_chains = q.n_chains; a.dim = q.dim; a.n_mh = q.n_mh; a.n_leapfrog = q.n_leapfrog;
  a.thin = q.thin; a.n_kept = q.n_kept(); a.draw_v0 = q.draw_v0 ? 1 : 0;
  a.n_adapt = q.n_adapt; a.init_da = (q.init_da & EBM_DA_INIT) ? 1 : 0; a.keep_open = (q.init_da & EBM_DA_OPEN) ? 1 : 0;
  // every double rounded once; gamma L and the two logs formed in double (as ghmc_adapt.hip)
  a.full_refresh = std::isinf(q.gamma) ? 1 : 0;
  a.eps0 = (float)q.eps0;
  a.gamma_l = a.full_refresh ? 0.0f : (float)(q.gamma * (double)q.n_leapfrog);
  a.temp = (float)q.temperature; a.sqrt_temp = (float)sqrt(q.temperature); a.beta = (float)(1.0 / q.temperature);
  a.delta = (float)q.target_accept; a.mu = (float)q.mu;
  a.log_eps_min = (float)log(q.eps_min); a.log_eps_max = (float)log(q.eps_max);
  fill_mass(a, m.mass);
  a.da = q.da; a.da_table = q.da_table; a.eps_trace = q.eps_trace; a.alpha_mean = q.alpha_mean;
  a.traj = q.traj; a.accept_mask = q.accept_mask; a.noise = q.noise; a.u = q.u;
  a.key = q.key(); a.step0 = q.offset;
  size_t smem = 0;
  plan_params(q.e, q.dim, geo, a.energy, a.param_floats, smem);
  const int64_t blocks = blocks_for(q.n_chains, geo);
  if (blocks > 0x7fffffffLL) return fail(EBM_EINVAL, "%s: too many chains for one launch", who);
  const dim3 grid((unsigned)blocks);
  for_kind(q.e.kind, [&](auto K) { ghmc_adapt_mass::launch_kind<decltype(K)::value>(geo, grid, smem, st, a); });
  return check_launch(who);
}

}  // namespace ebm
