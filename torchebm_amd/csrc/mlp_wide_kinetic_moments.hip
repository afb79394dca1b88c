// Running moments of the BAOAB and generalized-HMC walks on the wide MLP energy (ebm_kinetic_moments_mlp_f32): the walks of
// ebm_kinetic_mlp_chain_f32 and ebm_ghmc_mlp_chain_f32 with the Welford pairs of ebm_kinetic_moments_f32 kept in the caller's
// planes, in ONE launch (mlp_wide_kinetic_moments_body.h, mlp_wide_ghmc_moments_body.h; docs/design/kinetic_moments_mlp.md).
// Shapes: hidden width 64 / 128, dim <= 128 -- HT in {2, 4} x DT in {1 .. 4} at wide_mode(HT, DT), as the plain walks.  This unit
// holds the dispatch and the H = 64 BAOAB kernels; mlp_wide_kinetic_moments_h128.hip the H = 128 BAOAB kernels;
// mlp_wide_ghmc_moments.hip and mlp_wide_ghmc_moments_h128.hip the GHMC kernels.  Not built: H = 256, MODE 3 / 4, tables, a mass
// matrix.
#include "chain_launch.h"
#include "mlp_wide_kinetic_moments_body.h"
#include "mlp_wide_ghmc_moments_body.h"

namespace ebm {

int launch_kinetic_moments_mlp_wide_h128(const widemlp::WideKineticMomentsArgs& a, hipStream_t st, const char* who);  // mlp_wide_kinetic_moments_h128.hip
int launch_ghmc_moments_mlp_wide_h64(const widemlp::WideGhmcMomentsArgs& a, hipStream_t st, const char* who);         // mlp_wide_ghmc_moments.hip
int launch_ghmc_moments_mlp_wide_h128(const widemlp::WideGhmcMomentsArgs& a, hipStream_t st, const char* who);        // mlp_wide_ghmc_moments_h128.hip

int kinetic_moments_mlp_chain_launch(const KineticMomentsChainReq& q, hipStream_t st) {
  const char* who = "ebm_kinetic_moments_mlp_f32";
  if (int r = wide_mlp_check_shape(who, q.e.n_comp, q.dim)) return r;
  if (q.ghmc) {
    widemlp::WideGhmcMomentsArgs a{};
    a.x = q.x; a.v = q.v; a.n_chains = q.n_chains; a.dim = q.dim; a.k_steps = q.k_steps; a.burn_in = q.burn_in;
    a.half_len = q.half_len(); a.n_leapfrog = q.n_leapfrog; a.draw_v0 = q.draw_v0 ? 1 : 0;
    a.eps = q.eps; a.c1 = q.c1; a.c2 = q.c2; a.sqrt_temp = q.sqrt_temp; a.beta = q.beta;
    a.recip = q.recip; a.mom = q.mom; a.e_mom = q.e_mom; a.traj = q.traj; a.e_traj = q.e_traj;
    a.accept_mask = q.accept_mask; a.accept_count = q.accept_count; a.noise = q.noise; a.u = q.u;
    a.key = q.key(); a.step0 = q.offset;
    a.params = q.e.dev0;
    if (q.e.n_comp == 64) return launch_ghmc_moments_mlp_wide_h64(a, st, who);
    return launch_ghmc_moments_mlp_wide_h128(a, st, who);
  }
  widemlp::WideKineticMomentsArgs a{};
  a.x = q.x; a.v = q.v; a.n_chains = q.n_chains; a.dim = q.dim; a.k_steps = q.k_steps; a.burn_in = q.burn_in;
  a.half_len = q.half_len(); a.draw_v0 = q.draw_v0 ? 1 : 0;
  a.hh = q.hh; a.c1 = q.c1; a.c2 = q.c2; a.sqrt_temp = q.sqrt_temp;
  a.recip = q.recip; a.mom = q.mom; a.e_mom = q.e_mom; a.v2_mom = q.v2_mom; a.traj = q.traj; a.e_traj = q.e_traj;
  a.v_traj = q.v_traj; a.noise = q.noise;
  a.key = q.key(); a.step0 = q.offset;
  a.params = q.e.dev0;
  if (q.e.n_comp == 64) return widemlp::launch_walk_by_dim<widemlp::KineticMomentsWalk, 2>(a, st, who);
  return launch_kinetic_moments_mlp_wide_h128(a, st, who);
}

}  // namespace ebm
