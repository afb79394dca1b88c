// The kinetic / generalized-HMC running-moments kernels of ONE energy kind and ONE sampler (kinetic_moments_kernel.h).  The
// Makefile compiles moments_kinetic_unit.hip and moments_ghmc_unit.hip, which set EBM_KINETIC_MOMENTS_GHMC and include this
// source, once per kind (-DEBM_UNIT_KIND=...) into moments_kinetic_<kind>.o and moments_ghmc_<kind>.o, so that kinds and
// samplers build in parallel.
#include "kinetic_moments_kernel.h"

#ifndef EBM_KINETIC_MOMENTS_GHMC
#error "compile moments_kinetic_unit.hip or moments_ghmc_unit.hip, not this file"
#endif

namespace ebm {
namespace kinetic_moments {

#if EBM_KINETIC_MOMENTS_GHMC
template <int KIND>
void launch_ghmc_kind(const Geometry& geo, dim3 grid, size_t smem, hipStream_t st, const KineticMomentsArgs& a) {
  EBM_GEO_LAUNCH_NV1(moments_ghmc_chain, KIND, geo, grid, dim3(kBlock), smem, st, a);  // kinetic_moments.hip refuses wider rows
}
template void launch_ghmc_kind<EBM_UNIT_KIND>(const Geometry&, dim3, size_t, hipStream_t, const KineticMomentsArgs&);
#else
// the energy path is a compile-time switch, chosen by whether e_mom is NULL
template <int KIND>
void launch_baoab_kind(const Geometry& geo, dim3 grid, size_t smem, hipStream_t st, const KineticMomentsArgs& a) {
  if (a.e_mom) EBM_GEO_LAUNCH_NV1(moments_kinetic_chain_energy, KIND, geo, grid, dim3(kBlock), smem, st, a);
  else EBM_GEO_LAUNCH_NV1(moments_kinetic_chain, KIND, geo, grid, dim3(kBlock), smem, st, a);
}
template void launch_baoab_kind<EBM_UNIT_KIND>(const Geometry&, dim3, size_t, hipStream_t, const KineticMomentsArgs&);
#endif

}  // namespace kinetic_moments
}  // namespace ebm
