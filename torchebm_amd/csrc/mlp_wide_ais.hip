// Annealed importance sampling on the wide MLP energy (ebm_ais_mlp_chain_f32): the whole estimate -- the start draw, T weight
// updates, T Metropolis-corrected HMC transitions on the path energy, Philox draws, per-temperature accept counters -- in ONE
// launch, with the evaluation of mlp_wide_body.h inside the transition state machine (mlp_wide_ais_body.h; docs/design/ais_mlp.md).
// Shapes: hidden width 64 / 128, dim <= 128 -- HT in {2, 4} x DT in {1 .. 4} at wide_mode(HT, DT): split-bf16 images in LDS
// (MODE 2), fp32 weights in LDS at H = 128 above dim 64 (MODE 0).  This unit holds the H = 64 kernels and the dispatch,
// mlp_wide_ais_h128.hip the H = 128 kernels.  Not built: H = 256 (STREAM), the slab mode (MODE 3), a FAST variant, diagonal or
// scalar mass.
#include "chain_launch.h"
#include "mlp_wide_ais_body.h"

namespace ebm {

int launch_ais_mlp_wide_h128(const widemlp::WideAisArgs& a, hipStream_t st, const char* who);  // mlp_wide_ais_h128.hip

int ais_mlp_chain_launch(const AisChainReq& q, hipStream_t st) {
  const char* who = "ebm_ais_mlp_chain_f32";
  if (int r = wide_mlp_check_shape(who, q.e.n_comp, q.dim)) return r;
  widemlp::WideAisArgs a{};
  a.x = q.x; a.logw = q.logw; a.n_chains = q.n_chains; a.dim = q.dim; a.n_temps = q.n_temps; a.n_leapfrog = q.n_leapfrog;
  a.beta = q.beta; a.eps = q.eps; a.sigma0 = q.sigma0; a.inv_var0 = q.inv_var0;
  a.accept_mask = q.accept_mask; a.accept_counts = q.accept_counts;
  a.x0 = q.x0; a.p_noise = q.p_noise; a.u_accept = q.u_accept; a.key = q.key(); a.step0 = q.offset;
  a.params = q.e.dev0;
  if (q.e.n_comp == 64) return widemlp::launch_walk_by_dim<widemlp::AisWalk, 2>(a, st, who);
  return launch_ais_mlp_wide_h128(a, st, who);
}

}  // namespace ebm
