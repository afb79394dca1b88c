// Generalized HMC with a scalar or diagonal mass on the wide MLP energy (ebm_ghmc_mlp_chain_mass_f32): the walk of
// mlp_wide_ghmc.hip with the momentum as its carried plane -- the partial refresh, a Metropolis-corrected massed leapfrog
// trajectory of n_leapfrog + 1 evaluations, the flip on a reject, Philox draws, thinned trajectory, accept mask -- in ONE launch
// (mlp_wide_ghmc_mass_body.h; docs/design/mass_mlp.md).  The mass forms are LDS tables behind the unit-mass layout
// (mlp_wide_mass.h).  Shapes: the unit-mass walk's -- hidden width 64 / 128, dim <= 128, HT in {2, 4} x DT in {1 .. 4} at
// wide_mode(HT, DT).  This unit holds the H = 64 kernels and the dispatch, mlp_wide_ghmc_mass_h128.hip the H = 128 kernels.
// Not built: what mlp_wide_ghmc.hip does not build, a dense mass.
#include "chain_launch.h"
#include "mlp_wide_ghmc_mass_body.h"

namespace ebm {

int launch_ghmc_mass_mlp_wide_h128(const widemlp::WideGhmcMassArgs& a, hipStream_t st, const char* who);  // mlp_wide_ghmc_mass_h128.hip

int ghmc_mass_mlp_chain_launch(const GhmcMassChainReq& m, hipStream_t st) {
  const char* who = "ebm_ghmc_mlp_chain_mass_f32";
  const GhmcChainReq& q = m.chain;
  if (int r = wide_mlp_check_shape(who, q.e.n_comp, q.dim)) return r;
  widemlp::WideGhmcMassArgs a{};
  a.x = q.x; a.v = q.v; a.n_chains = q.n_chains; a.dim = q.dim; a.n_mh = q.n_mh; a.n_leapfrog = q.n_leapfrog;
  a.thin = q.thin; a.n_kept = q.n_kept(); a.draw_v0 = q.draw_v0 ? 1 : 0;
  a.eps = q.eps; a.c1 = q.c1; a.c2 = q.c2; a.sqrt_temp = q.sqrt_temp; a.beta = q.beta;
  fill_mass(a, m.mass);
  a.traj = q.traj; a.accept_mask = q.accept_mask; a.noise = q.noise; a.u = q.u;
  a.key = q.key(); a.step0 = q.offset;
  a.params = q.e.dev0;
  if (q.e.n_comp == 64) return widemlp::launch_massed_walk_by_dim<widemlp::GhmcMassWalk, 2>(a, st, who);
  return launch_ghmc_mass_mlp_wide_h128(a, st, who);
}

}  // namespace ebm
