// Underdamped Langevin, BAOAB, on the three-hidden-layer SiLU MLP energy at hidden width 64: the launcher behind
// ebm_kinetic_chain_mlp3_f32 (include/ebm_hip_mlp3_kinetic.h; the entry and its refusals are api.hip's, beside the other
// underdamped-Langevin entries whose constants it shares) and the three instantiations of mlp3_kinetic_body.h's kernel
// (DT = 1 / 2 / 4 for dim <= 32 / 64 / 128; docs/design/mlp3_kinetic.md).
#include "mlp3_kinetic_launch.h"
#include "mlp3_kinetic_body.h"

namespace ebm {

int kinetic_mlp3_chain_launch(const KineticChainReq& q, hipStream_t st) {
  const char* who = "ebm_kinetic_chain_mlp3_f32";
  if (q.e.n_comp != 64 || q.dim < 1 || q.dim > 128)  // (the entry's own refusal, repeated where the instantiation is chosen)
    return fail(EBM_EDIM, "%s: hidden width %d, dim %d (the kernel takes hidden width 64 with dim 1 .. 128)", who, q.e.n_comp, q.dim);
  mlp3::KineticArgs a{};
  a.x = q.x; a.v = q.v; a.n_chains = q.n_chains; a.dim = q.dim; a.k_steps = q.k_steps;
  a.thin = q.thin; a.n_kept = q.n_kept(); a.draw_v0 = q.draw_v0 ? 1 : 0;
  a.hh = q.hh; a.c1 = q.c1; a.c2 = q.c2; a.sqrt_temp = q.sqrt_temp;
  a.traj = q.traj; a.noise = q.noise;
  a.key = q.key(); a.step0 = q.offset;
  a.params = static_cast<const float*>(q.e.dev0);
  if (q.dim <= 32) return mlp3::launch_kinetic<1>(a, st, who);
  if (q.dim <= 64) return mlp3::launch_kinetic<2>(a, st, who);
  return mlp3::launch_kinetic<4>(a, st, who);
}

}  // namespace ebm
