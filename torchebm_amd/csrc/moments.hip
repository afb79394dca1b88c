// Per-chain running moments (ebm_chain_moments_f32): geometry, refusals and dispatch to the per-energy units
// (moments_unit.hip, one object per kind and sampler; the kernels: moments_kernel.h).
#include "moments_kernel.h"

namespace ebm {

// The refusal that depends on the lane geometry (no launch, no device access): ebm_chain_moments_f32 calls this in front of
// its early return for an empty call, so it needs no GPU.
int moments_check_geometry(int32_t dim) {
  rows::Geometry geo;
  if (!rows::pick_geometry(dim, geo) || geo.NV != 1)
    return fail(EBM_EDIM, "ebm_chain_moments_f32: dim %d > 256 is not supported (one vector per lane)", dim);
  return 0;
}

int moments_chain_launch(const MomentsChainReq& q, hipStream_t st) {
  using namespace rows;
  const char* who = "ebm_chain_moments_f32";
  if (int r = moments_check_geometry(q.dim)) return r;
  Geometry geo;
  pick_geometry(q.dim, geo);
  moments::MomentsArgs a{};
  a.x = q.x; a.n_chains = q.n_chains; a.dim = q.dim; a.k_steps = q.k_steps; a.burn_in = q.burn_in;
  a.half_len = q.half_len(); a.n_leapfrog = q.n_leapfrog;
  a.eta = q.eta; a.sqrt_eta = q.sqrt_eta; a.noise_coef = q.noise_coef; a.eps = q.eps;
  a.recip = q.recip; a.mom = q.mom; a.e_mom = q.e_mom; a.traj = q.traj; a.e_traj = q.e_traj;
  a.accept_mask = q.accept_mask; a.accept_count = q.accept_count; a.noise = q.noise_or_p; a.u = q.u;
  a.key = q.key(); a.step0 = q.offset;
  size_t smem = 0;
  plan_params(q.e, q.dim, geo, a.energy, a.param_floats, smem);
  const int64_t blocks = blocks_for(q.n_chains, geo);
  if (blocks > 0x7fffffffLL) return fail(EBM_EINVAL, "%s: too many chains for one launch", who);
  const dim3 grid((unsigned)blocks);
  if (q.hmc) for_kind(q.e.kind, [&](auto K) { moments::launch_hmc_kind<decltype(K)::value>(geo, grid, smem, st, a); });
  else for_kind(q.e.kind, [&](auto K) { moments::launch_langevin_kind<decltype(K)::value>(geo, grid, smem, st, a); });
  return check_launch(who);
}

}  // namespace ebm
