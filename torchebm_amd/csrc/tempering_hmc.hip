// Replica-exchange HMC (ebm_tempering_hmc_chain_f32): geometry, refusals and dispatch to the per-energy units
// (tempering_hmc_unit.hip, one object per kind; the kernel: tempering_hmc_kernel.h).
#include "tempering_hmc_kernel.h"

namespace ebm {

// The refusals that depend on the lane geometry (no launch, no device access): ebm_tempering_hmc_chain_f32 calls this in
// front of its early return for an empty call, so they need no GPU.
int tempering_hmc_check_geometry(int32_t n_replicas, int32_t dim) {
  const char* who = "ebm_tempering_hmc_chain_f32";
  rows::Geometry geo;
  if (!rows::pick_geometry(dim, geo) || geo.NV != 1)
    return fail(EBM_EDIM, "%s: dim %d > 256 is not supported (one vector per lane)", who, dim);
  if (n_replicas * geo.G > rows::kBlock)
    return fail(EBM_EDIM, "%s: a ladder of %d replicas at dim %d (%d lanes per replica) does not fit one workgroup of %d lanes", who,
                n_replicas, dim, geo.G, rows::kBlock);
  return 0;
}

int tempering_hmc_chain_launch(const TemperingHmcChainReq& q, hipStream_t st) {
  using namespace rows;
  const char* who = "ebm_tempering_hmc_chain_f32";
  if (int r = tempering_hmc_check_geometry(q.n_replicas, q.dim)) return r;
  Geometry geo;
  pick_geometry(q.dim, geo);
  tempering_hmc::TemperHmcArgs a{};
  a.x = q.x; a.n_ladders = q.n_ladders; a.R = q.n_replicas; a.dim = q.dim; a.n_mh = q.n_mh; a.n_leapfrog = q.n_leapfrog;
  a.eps = q.eps; a.sqrt_temp = q.sqrt_temp; a.beta = q.beta;
  a.swap_every = q.swap_every; a.thin = q.thin; a.n_kept = q.n_kept(); a.traj = q.traj;
  a.accept_mask = q.accept_mask; a.accept_counts = q.accept_counts; a.swap_counts = q.swap_counts;
  a.p_noise = q.p_noise; a.u_accept = q.u_accept; a.u_swap = q.u_swap; a.key = q.key(); a.step0 = q.offset;
  size_t smem = 0;
  plan_params(q.e, q.dim, geo, a.energy, a.param_floats, smem);
  const int64_t blocks = ladder::plan(geo, q.n_replicas, q.n_ladders, smem, a.table_offset_floats);
  smem += 64 * sizeof(uint32_t);  // behind the energy table: the per-slot accept counters (n_replicas <= 64)
  if (blocks > 0x7fffffffLL) return fail(EBM_EINVAL, "%s: too many ladders for one launch", who);
  const dim3 grid((unsigned)blocks);
  for_kind(q.e.kind, [&](auto K) { tempering_hmc::launch_kind<decltype(K)::value>(geo, grid, smem, st, a); });
  return check_launch(who);
}

}  // namespace ebm
