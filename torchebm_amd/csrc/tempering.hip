// Replica-exchange Langevin (ebm_tempering_chain_f32): geometry, refusals and dispatch to the per-energy units
// (tempering_unit.hip, one object per kind; the kernel: tempering_kernel.h).
#include "tempering_kernel.h"

namespace ebm {

// The refusals that depend on the lane geometry (no launch, no device access): ebm_tempering_chain_f32 calls this in front
// of its early return for an empty call, so they need no GPU.
int tempering_check_geometry(int32_t n_replicas, int32_t dim) {
  const char* who = "ebm_tempering_chain_f32";
  rows::Geometry geo;
  if (!rows::pick_geometry(dim, geo)) return fail(EBM_EDIM, "%s: dim %d > 1024 is not supported", who, dim);
  if (n_replicas * geo.G > rows::kBlock)
    return fail(EBM_EDIM, "%s: a ladder of %d replicas at dim %d (%d lanes per replica) does not fit one workgroup of %d lanes", who,
                n_replicas, dim, geo.G, rows::kBlock);
  return 0;
}

int tempering_chain_launch(const TemperingChainReq& q, hipStream_t st) {
  using namespace rows;
  const char* who = "ebm_tempering_chain_f32";
  if (int r = tempering_check_geometry(q.n_replicas, q.dim)) return r;
  Geometry geo;
  pick_geometry(q.dim, geo);
  tempering::TemperArgs a{};
  a.x = q.x; a.n_ladders = q.n_ladders; a.R = q.n_replicas; a.dim = q.dim; a.k_steps = q.k_steps;
  a.eta = q.eta; a.sqrt_eta = q.sqrt_eta; a.noise_coef = q.noise_coef; a.beta = q.beta;
  a.swap_every = q.swap_every; a.thin = q.thin; a.n_kept = q.n_kept(); a.traj = q.traj; a.swap_counts = q.swap_counts;
  a.noise = q.noise; a.u = q.u; a.key = q.key(); a.step0 = q.offset;
  size_t smem = 0;
  plan_params(q.e, q.dim, geo, a.energy, a.param_floats, smem);
  const int64_t blocks = ladder::plan(geo, q.n_replicas, q.n_ladders, smem, a.table_offset_floats);
  if (blocks > 0x7fffffffLL) return fail(EBM_EINVAL, "%s: too many ladders for one launch", who);
  const dim3 grid((unsigned)blocks);
  for_kind(q.e.kind, [&](auto K) { tempering::launch_kind<decltype(K)::value>(geo, grid, smem, st, a); });
  return check_launch(who);
}

}  // namespace ebm
