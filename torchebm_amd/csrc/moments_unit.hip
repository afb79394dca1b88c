// The running-moments kernels of ONE energy kind and ONE sampler (moments_kernel.h).  The Makefile compiles
// moments_langevin_unit.hip and moments_hmc_unit.hip, which set EBM_MOMENTS_HMC and include this source, once per kind
// (-DEBM_UNIT_KIND=...) into moments_langevin_<kind>.o and moments_hmc_<kind>.o, so that kinds and samplers build in parallel.
#include "moments_kernel.h"

#ifndef EBM_MOMENTS_HMC
#error "compile moments_langevin_unit.hip or moments_hmc_unit.hip, not this file"
#endif

namespace ebm {
namespace moments {

#if EBM_MOMENTS_HMC
template <int KIND>
void launch_hmc_kind(const Geometry& geo, dim3 grid, size_t smem, hipStream_t st, const MomentsArgs& a) {
  EBM_GEO_LAUNCH_NV1(moments_hmc_chain, KIND, geo, grid, dim3(kBlock), smem, st, a);  // moments.hip refuses wider rows
}
template void launch_hmc_kind<EBM_UNIT_KIND>(const Geometry&, dim3, size_t, hipStream_t, const MomentsArgs&);
#else
// the energy path is a compile-time switch, chosen by whether e_mom is NULL
template <int KIND>
void launch_langevin_kind(const Geometry& geo, dim3 grid, size_t smem, hipStream_t st, const MomentsArgs& a) {
  if (a.e_mom) EBM_GEO_LAUNCH_NV1(moments_langevin_chain_energy, KIND, geo, grid, dim3(kBlock), smem, st, a);
  else EBM_GEO_LAUNCH_NV1(moments_langevin_chain, KIND, geo, grid, dim3(kBlock), smem, st, a);
}
template void launch_langevin_kind<EBM_UNIT_KIND>(const Geometry&, dim3, size_t, hipStream_t, const MomentsArgs&);
#endif

}  // namespace moments
}  // namespace ebm
