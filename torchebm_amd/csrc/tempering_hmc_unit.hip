// The replica-exchange HMC kernels of ONE energy kind (tempering_hmc_kernel.h).  The Makefile compiles this source once per
// kind (-DEBM_UNIT_KIND=...) into tempering_hmc_<kind>.o, so that the energies build in parallel.
#include "tempering_hmc_kernel.h"

namespace ebm {
namespace tempering_hmc {

template <int KIND>
void launch_kind(const Geometry& geo, dim3 grid, size_t smem, hipStream_t st, const TemperHmcArgs& a) {
  EBM_GEO_LAUNCH_NV1(tempering_hmc_ladder_chain, KIND, geo, grid, dim3(kBlock), smem, st, a);  // tempering_hmc.hip refuses wider rows
}
template void launch_kind<EBM_UNIT_KIND>(const Geometry&, dim3, size_t, hipStream_t, const TemperHmcArgs&);

}  // namespace tempering_hmc
}  // namespace ebm
