// Replica-exchange HMC on the wide MLP energy (ebm_tempering_hmc_mlp_chain_f32): n_mh transitions of every slot of every ladder --
// the slot's velocity draw, a Metropolis-corrected leapfrog trajectory of n_leapfrog + 1 evaluations of mlp_wide_body.h, the swap
// events between neighbouring lanes, Philox draws, the thinned slot-0 trajectory, accept mask and counters -- in ONE launch
// (mlp_wide_tempering_body.h; docs/design/tempering_hmc_mlp.md).
// Shapes: hidden width 64 / 128, dim <= 128 -- HT in {2, 4} x DT in {1 .. 4} at wide_mode(HT, DT): split-bf16 images in LDS
// (MODE 2), fp32 weights in LDS at H = 128 above dim 64 (MODE 0); ladders of 2, 4, 8, 16 or 32 slots, whole ladders per wave.
// This unit holds the H = 64 kernels and the dispatch, mlp_wide_tempering_h128.hip the H = 128 kernels.  Not built: other ladder
// lengths (idle lanes per wave), H = 256 (STREAM), the slab mode (MODE 3), the THIN mode (MODE 4), FAST variants, diagnostics
// records, tables.
#include "chain_launch.h"
#include "mlp_wide_tempering_body.h"

namespace ebm {

int launch_tempering_mlp_wide_h128(const widemlp::WideTemperArgs& a, hipStream_t st, const char* who);  // mlp_wide_tempering_h128.hip

int tempering_hmc_mlp_chain_launch(const TemperingHmcChainReq& q, hipStream_t st) {
  const char* who = "ebm_tempering_hmc_mlp_chain_f32";
  if (int r = wide_mlp_check_ladder_shape(who, q.e.n_comp, q.dim, q.n_replicas)) return r;
  widemlp::WideTemperArgs a{};
  a.x = q.x; a.n_chains = q.n_ladders * (int64_t)q.n_replicas; a.R = q.n_replicas; a.dim = q.dim; a.n_mh = q.n_mh;
  a.n_leapfrog = q.n_leapfrog; a.swap_every = q.swap_every; a.thin = q.thin; a.n_kept = q.n_kept();
  a.eps = q.eps; a.sqrt_temp = q.sqrt_temp; a.beta = q.beta;
  a.traj = q.traj; a.accept_mask = q.accept_mask; a.accept_counts = q.accept_counts; a.swap_counts = q.swap_counts;
  a.p_noise = q.p_noise; a.u_accept = q.u_accept; a.u_swap = q.u_swap;
  a.key = q.key(); a.step0 = q.offset;
  a.params = q.e.dev0;
  if (q.e.n_comp == 64) return widemlp::launch_walk_by_dim<widemlp::TemperWalk, 2>(a, st, who);
  return launch_tempering_mlp_wide_h128(a, st, who);
}

}  // namespace ebm
