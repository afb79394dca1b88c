// Underdamped Langevin, BAOAB, on the wide MLP energy (ebm_kinetic_mlp_chain_f32): k_steps steps of a walker per chain that keeps
// position, velocity and gradient in registers around the evaluation of mlp_wide_body.h -- k_steps + 1 evaluations, Philox draws,
// thinned trajectory -- in ONE launch (mlp_wide_kinetic_body.h; docs/design/kinetic_mlp.md).
// Shapes: hidden width 64 / 128, dim <= 128 -- HT in {2, 4} x DT in {1 .. 4} at wide_mode(HT, DT): split-bf16 images in LDS
// (MODE 2), fp32 weights in LDS at H = 128 above dim 64 (MODE 0).  This unit holds the H = 64 kernels and the dispatch,
// mlp_wide_kinetic_h128.hip the H = 128 kernels.  Not built: H = 256 (STREAM), the slab mode (MODE 3), the THIN mode (MODE 4),
// FAST variants, diagnostics records, clamp, tables.  A scalar or diagonal mass is a kernel family of its own,
// mlp_wide_kinetic_mass.hip: this unit never sees a mass.
#include "chain_launch.h"
#include "mlp_wide_kinetic_body.h"

namespace ebm {

int launch_kinetic_mlp_wide_h128(const widemlp::WideKineticArgs& a, hipStream_t st, const char* who);  // mlp_wide_kinetic_h128.hip

int kinetic_mlp_chain_launch(const KineticChainReq& q, hipStream_t st) {
  const char* who = "ebm_kinetic_mlp_chain_f32";
  if (int r = wide_mlp_check_shape(who, q.e.n_comp, q.dim)) return r;
  widemlp::WideKineticArgs a{};
  a.x = q.x; a.v = q.v; a.n_chains = q.n_chains; a.dim = q.dim; a.k_steps = q.k_steps;
  a.thin = q.thin; a.n_kept = q.n_kept(); a.draw_v0 = q.draw_v0 ? 1 : 0;
  a.hh = q.hh; a.c1 = q.c1; a.c2 = q.c2; a.sqrt_temp = q.sqrt_temp;
  a.traj = q.traj; a.noise = q.noise;
  a.key = q.key(); a.step0 = q.offset;
  a.params = q.e.dev0;
  if (q.e.n_comp == 64) return widemlp::launch_walk_by_dim<widemlp::KineticWalk, 2>(a, st, who);
  return launch_kinetic_mlp_wide_h128(a, st, who);
}

}  // namespace ebm
