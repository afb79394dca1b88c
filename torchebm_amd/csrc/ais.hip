// Annealed importance sampling (ebm_ais_chain_f32): geometry, refusals and dispatch to the per-energy units
// (ais_unit.hip, one object per kind; the kernel: ais_kernel.h).
#include "ais_kernel.h"

namespace ebm {

// The refusal that depends on the lane geometry (no launch, no device access): ebm_ais_chain_f32 calls this in front of its
// early return for an empty call, so it needs no GPU.
int ais_check_geometry(int32_t dim) {
  rows::Geometry geo;
  if (!rows::pick_geometry(dim, geo) || geo.NV != 1)
    return fail(EBM_EDIM, "ebm_ais_chain_f32: dim %d > 256 is not supported (one vector per lane)", dim);
  return 0;
}

int ais_chain_launch(const AisChainReq& q, hipStream_t st) {
  using namespace rows;
  const char* who = "ebm_ais_chain_f32";
  if (int r = ais_check_geometry(q.dim)) return r;
  Geometry geo;
  pick_geometry(q.dim, geo);
  ais::AisArgs a{};
  a.x = q.x; a.logw = q.logw; a.n_chains = q.n_chains; a.dim = q.dim; a.n_temps = q.n_temps; a.n_leapfrog = q.n_leapfrog;
  a.beta = q.beta; a.eps = q.eps; a.sigma0 = q.sigma0; a.inv_var0 = q.inv_var0;
  a.accept_mask = q.accept_mask; a.accept_counts = q.accept_counts;
  a.x0 = q.x0; a.p_noise = q.p_noise; a.u_accept = q.u_accept; a.key = q.key(); a.step0 = q.offset;
  size_t smem = 0;
  plan_params(q.e, q.dim, geo, a.energy, a.param_floats, smem);
  const int64_t blocks = blocks_for(q.n_chains, geo);
  if (blocks > 0x7fffffffLL) return fail(EBM_EINVAL, "%s: too many chains for one launch", who);
  const dim3 grid((unsigned)blocks);
  for_kind(q.e.kind, [&](auto K) { ais::launch_kind<decltype(K)::value>(geo, grid, smem, st, a); });
  return check_launch(who);
}

}  // namespace ebm
