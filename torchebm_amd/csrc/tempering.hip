// Replica-exchange Langevin (ebm_tempering_chain_f32): geometry, refusals and dispatch to the per-energy units
// (tempering_<energy>.hip; the kernel: tempering_kernel.h).
#include "tempering_kernel.h"

namespace ebm {
namespace tempering {
void launch_double_well(const rows::Geometry&, dim3, size_t, hipStream_t, const TemperArgs&);
void launch_harmonic(const rows::Geometry&, dim3, size_t, hipStream_t, const TemperArgs&);
void launch_gaussian(const rows::Geometry&, dim3, size_t, hipStream_t, const TemperArgs&);
void launch_gmm(const rows::Geometry&, dim3, size_t, hipStream_t, const TemperArgs&);
void launch_rosenbrock(const rows::Geometry&, dim3, size_t, hipStream_t, const TemperArgs&);
void launch_ackley(const rows::Geometry&, dim3, size_t, hipStream_t, const TemperArgs&);
void launch_rastrigin(const rows::Geometry&, dim3, size_t, hipStream_t, const TemperArgs&);
}  // namespace tempering

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
  a.table_offset_floats = (int)(smem / sizeof(float));
  smem += (size_t)(kBlock / geo.G) * sizeof(float);  // the energy table: one float per lane group
  const int lpb = (kBlock / geo.G) / q.n_replicas;
  const int64_t blocks = ceil_div64(q.n_ladders, lpb);
  if (blocks > 0x7fffffffLL) return fail(EBM_EINVAL, "%s: too many ladders for one launch", who);
  const dim3 grid((unsigned)blocks);
  switch (q.e.kind) {
    case EBM_ENERGY_DOUBLE_WELL: tempering::launch_double_well(geo, grid, smem, st, a); break;
    case EBM_ENERGY_HARMONIC:    tempering::launch_harmonic(geo, grid, smem, st, a); break;
    case EBM_ENERGY_GAUSSIAN:    tempering::launch_gaussian(geo, grid, smem, st, a); break;
    case EBM_ENERGY_ROSENBROCK:  tempering::launch_rosenbrock(geo, grid, smem, st, a); break;
    case EBM_ENERGY_ACKLEY:      tempering::launch_ackley(geo, grid, smem, st, a); break;
    case EBM_ENERGY_RASTRIGIN:   tempering::launch_rastrigin(geo, grid, smem, st, a); break;
    default:                     tempering::launch_gmm(geo, grid, smem, st, a); break;
  }
  return check_launch(who);
}

}  // namespace ebm
