// Underdamped Langevin, BAOAB, with a mass (ebm_kinetic_chain_mass_f32): geometry and dispatch to the per-energy units
// (kinetic_mass_unit.hip, one object per kind; the kernel: kinetic_mass_kernel.h).  The geometry refusal is kinetic.hip's.
#include "kinetic_mass_kernel.h"

namespace ebm {

int kinetic_mass_chain_launch(const KineticMassChainReq& m, hipStream_t st) {
  using namespace rows;
  const char* who = "ebm_kinetic_chain_mass_f32";
  const KineticChainReq& q = m.chain;
  if (int r = kinetic_check_geometry(q.dim)) return r;
  Geometry geo;
  pick_geometry(q.dim, geo);
  kinetic_mass::KineticMassArgs a{};
  a.x = q.x; a.v = q.v; a.n_chains = q.n_chains; a.dim = q.dim; a.k_steps = q.k_steps;
  a.thin = q.thin; a.n_kept = q.n_kept(); a.draw_v0 = q.draw_v0 ? 1 : 0;
  a.hh = q.hh; a.c1 = q.c1; a.c2 = q.c2; a.sqrt_temp = q.sqrt_temp;
  fill_mass(a, m.mass);
  a.traj = q.traj; a.noise = q.noise;
  a.key = q.key(); a.step0 = q.offset;
  size_t smem = 0;
  plan_params(q.e, q.dim, geo, a.energy, a.param_floats, smem);
  const int64_t blocks = blocks_for(q.n_chains, geo);
  if (blocks > 0x7fffffffLL) return fail(EBM_EINVAL, "%s: too many chains for one launch", who);
  const dim3 grid((unsigned)blocks);
  for_kind(q.e.kind, [&](auto K) { kinetic_mass::launch_kind<decltype(K)::value>(geo, grid, smem, st, a); });
  return check_launch(who);
}

}  // namespace ebm
