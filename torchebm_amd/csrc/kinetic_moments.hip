// Running moments of the BAOAB and generalized-HMC walkers (ebm_kinetic_moments_f32): geometry, refusals and dispatch to the
// per-energy units (kinetic_moments_unit.hip, one object per kind and sampler; the kernels: kinetic_moments_kernel.h).
#include "kinetic_moments_kernel.h"

namespace ebm {

// The refusal that depends on the lane geometry (no launch, no device access): ebm_kinetic_moments_f32 calls this in front of
// its early return for an empty call, so it needs no GPU.
int kinetic_moments_check_geometry(int32_t dim) {
  rows::Geometry geo;
  if (dim < 1 || !rows::pick_geometry(dim, geo) || geo.NV != 1)
    return fail(EBM_EDIM, "ebm_kinetic_moments_f32: dim %d outside 1 .. 256 is not supported (one vector per lane)", dim);
  return 0;
}

int kinetic_moments_chain_launch(const KineticMomentsChainReq& q, hipStream_t st) {
  using namespace rows;
  const char* who = "ebm_kinetic_moments_f32";
  if (int r = kinetic_moments_check_geometry(q.dim)) return r;
  Geometry geo;
  pick_geometry(q.dim, geo);
  kinetic_moments::KineticMomentsArgs a{};
  a.x = q.x; a.v = q.v; a.n_chains = q.n_chains; a.dim = q.dim; a.k_steps = q.k_steps; a.burn_in = q.burn_in;
  a.half_len = q.half_len(); a.n_leapfrog = q.n_leapfrog; a.draw_v0 = q.draw_v0 ? 1 : 0;
  a.hh = q.hh; a.eps = q.eps; a.beta = q.beta; a.c1 = q.c1; a.c2 = q.c2; a.sqrt_temp = q.sqrt_temp;
  a.recip = q.recip; a.mom = q.mom; a.e_mom = q.e_mom; a.v2_mom = q.v2_mom;
  a.traj = q.traj; a.e_traj = q.e_traj; a.v_traj = q.v_traj;
  a.accept_mask = q.accept_mask; a.accept_count = q.accept_count; a.noise = q.noise; a.u = q.u;
  a.key = q.key(); a.step0 = q.offset;
  size_t smem = 0;
  plan_params(q.e, q.dim, geo, a.energy, a.param_floats, smem);
  const int64_t blocks = blocks_for(q.n_chains, geo);
  if (blocks > 0x7fffffffLL) return fail(EBM_EINVAL, "%s: too many chains for one launch", who);
  const dim3 grid((unsigned)blocks);
  if (q.ghmc) for_kind(q.e.kind, [&](auto K) { kinetic_moments::launch_ghmc_kind<decltype(K)::value>(geo, grid, smem, st, a); });
  else for_kind(q.e.kind, [&](auto K) { kinetic_moments::launch_baoab_kind<decltype(K)::value>(geo, grid, smem, st, a); });
  return check_launch(who);
}

}  // namespace ebm
