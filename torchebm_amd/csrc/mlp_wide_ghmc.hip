// Generalized HMC on the wide MLP energy (ebm_ghmc_mlp_chain_f32): n_mh transitions of a walker per chain -- the partial velocity
// refresh, a Metropolis-corrected leapfrog trajectory of n_leapfrog + 1 evaluations of mlp_wide_body.h, the flip on a reject,
// Philox draws, thinned trajectory, accept mask -- in ONE launch (mlp_wide_ghmc_body.h; docs/design/ghmc_mlp.md).
// Shapes: hidden width 64 / 128, dim <= 128 -- HT in {2, 4} x DT in {1 .. 4} at wide_mode(HT, DT): split-bf16 images in LDS
// (MODE 2), fp32 weights in LDS at H = 128 above dim 64 (MODE 0).  This unit holds the H = 64 kernels and the dispatch,
// mlp_wide_ghmc_h128.hip the H = 128 kernels.  Not built: H = 256 (STREAM), the slab mode (MODE 3), the THIN mode (MODE 4),
// FAST variants, diagnostics records, tables.  A scalar or diagonal mass is a kernel family of its own,
// mlp_wide_ghmc_mass.hip: this unit never sees a mass.
#include "chain_launch.h"
#include "mlp_wide_ghmc_body.h"

namespace ebm {

int launch_ghmc_mlp_wide_h128(const widemlp::WideGhmcArgs& a, hipStream_t st, const char* who);  // mlp_wide_ghmc_h128.hip

int ghmc_mlp_chain_launch(const GhmcChainReq& q, hipStream_t st) {
  const char* who = "ebm_ghmc_mlp_chain_f32";
  if (int r = wide_mlp_check_shape(who, q.e.n_comp, q.dim)) return r;
  widemlp::WideGhmcArgs a{};
  a.x = q.x; a.v = q.v; a.n_chains = q.n_chains; a.dim = q.dim; a.n_mh = q.n_mh; a.n_leapfrog = q.n_leapfrog;
  a.thin = q.thin; a.n_kept = q.n_kept(); a.draw_v0 = q.draw_v0 ? 1 : 0;
  a.eps = q.eps; a.c1 = q.c1; a.c2 = q.c2; a.sqrt_temp = q.sqrt_temp; a.beta = q.beta;
  a.traj = q.traj; a.accept_mask = q.accept_mask; a.noise = q.noise; a.u = q.u;
  a.key = q.key(); a.step0 = q.offset;
  a.params = q.e.dev0;
  if (q.e.n_comp == 64) return widemlp::launch_walk_by_dim<widemlp::GhmcWalk, 2>(a, st, who);
  return launch_ghmc_mlp_wide_h128(a, st, who);
}

}  // namespace ebm
