// Replica-exchange Langevin on the wide MLP energy (ebm_tempering_mlp_chain_f32): k_steps Euler-Maruyama steps of every slot of
// every ladder -- one evaluation of mlp_wide_body.h per step, the swap events between neighbouring lanes on that evaluation's
// energies, Philox draws, the thinned slot-0 trajectory and the swap counters -- in ONE launch
// (mlp_wide_tempering_langevin_body.h; docs/design/tempering_mlp.md).
// Shapes: hidden width 64 / 128, dim <= 128 -- HT in {2, 4} x DT in {1 .. 4} at wide_mode(HT, DT): split-bf16 images in LDS
// (MODE 2), fp32 weights in LDS at H = 128 above dim 64 (MODE 0); ladders of 2, 4, 8, 16 or 32 slots, whole ladders per wave.
// This unit holds the dispatch and the H = 64 kernels, mlp_wide_tempering_langevin_h128.hip the H = 128 kernels.
// Not built: other ladder lengths (idle lanes per wave), H = 256 (STREAM), the slab mode (MODE 3), the THIN mode (MODE 4), FAST
// variants, a clamp, diagnostics records, tables.
#include "chain_launch.h"
#include "mlp_wide_tempering_langevin_body.h"

namespace ebm {

int launch_tempering_langevin_mlp_wide_h128(const widemlp::WideTemperLangevinArgs& a, hipStream_t st, const char* who);  // mlp_wide_tempering_langevin_h128.hip

int tempering_mlp_chain_launch(const TemperingChainReq& q, hipStream_t st) {
  const char* who = "ebm_tempering_mlp_chain_f32";
  if (int r = wide_mlp_check_ladder_shape(who, q.e.n_comp, q.dim, q.n_replicas)) return r;
  widemlp::WideTemperLangevinArgs a{};
  a.x = q.x; a.n_chains = q.n_ladders * (int64_t)q.n_replicas; a.R = q.n_replicas; a.dim = q.dim; a.k_steps = q.k_steps;
  a.swap_every = q.swap_every; a.thin = q.thin; a.n_kept = q.n_kept();
  a.eta = q.eta; a.sqrt_eta = q.sqrt_eta; a.noise_coef = q.noise_coef; a.beta = q.beta;
  a.traj = q.traj; a.swap_counts = q.swap_counts; a.noise = q.noise; a.u = q.u;
  a.key = q.key(); a.step0 = q.offset;
  a.params = q.e.dev0;
  if (q.e.n_comp == 64) return widemlp::launch_walk_by_dim<widemlp::TemperLangevinWalk, 2>(a, st, who);
  return launch_tempering_langevin_mlp_wide_h128(a, st, who);
}

}  // namespace ebm
