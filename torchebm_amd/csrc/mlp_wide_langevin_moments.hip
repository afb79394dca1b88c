// Running moments of the Euler-Maruyama walk on the wide MLP energy (ebm_chain_moments_mlp_f32): the update of
// ebm_langevin_chain_f32 without clamp with the Welford pairs of ebm_chain_moments_f32 kept in the caller's planes, in ONE launch
// (mlp_wide_langevin_moments_body.h; docs/design/langevin_moments_mlp.md).  Shapes: hidden width 64 / 128, dim <= 128 -- HT in
// {2, 4} x DT in {1 .. 4} at wide_mode(HT, DT), as the other walks.  This unit holds the dispatch and the H = 64
// kernels; mlp_wide_langevin_moments_h128.hip the H = 128 kernels.  Not built: H = 256, MODE 3 / 4, tables, a clamp.
#include "chain_launch.h"
#include "mlp_wide_langevin_moments_body.h"

namespace ebm {

int launch_langevin_moments_mlp_wide_h128(const widemlp::WideLangevinMomentsArgs& a, hipStream_t st, const char* who);  // mlp_wide_langevin_moments_h128.hip

int langevin_moments_mlp_chain_launch(const LangevinMomentsChainReq& q, hipStream_t st) {
  const char* who = "ebm_chain_moments_mlp_f32";
  if (int r = wide_mlp_check_shape(who, q.e.n_comp, q.dim)) return r;
  widemlp::WideLangevinMomentsArgs a{};
  a.x = q.x; a.n_chains = q.n_chains; a.dim = q.dim; a.k_steps = q.k_steps; a.burn_in = q.burn_in;
  a.half_len = q.half_len();
  a.eta = q.eta; a.sqrt_eta = q.sqrt_eta; a.noise_coef = q.noise_coef;
  a.recip = q.recip; a.mom = q.mom; a.e_mom = q.e_mom; a.traj = q.traj; a.e_traj = q.e_traj; a.noise = q.noise;
  a.key = q.key(); a.step0 = q.offset;
  a.params = q.e.dev0;
  if (q.e.n_comp == 64) return widemlp::launch_walk_by_dim<widemlp::LangevinMomentsWalk, 2>(a, st, who);
  return launch_langevin_moments_mlp_wide_h128(a, st, who);
}

}  // namespace ebm
