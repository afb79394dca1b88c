// The massed adapting generalized-HMC kernels of ONE energy kind (ghmc_adapt_mass_kernel.h).  The Makefile compiles this source
// once per kind (-DEBM_UNIT_KIND=...) into ghmc_adapt_mass_<kind>.o, so that the kinds build in parallel.
#include "ghmc_adapt_mass_kernel.h"

namespace ebm {
namespace ghmc_adapt_mass {

template <int KIND>
void launch_kind(const Geometry& geo, dim3 grid, size_t smem, hipStream_t st, const GhmcAdaptMassArgs& a) {
  EBM_GEO_LAUNCH_NV1(ghmc_adapt_mass_chain, KIND, geo, grid, dim3(kBlock), smem, st, a);  // ghmc_adapt_mass.hip refuses wider rows
}
template void launch_kind<EBM_UNIT_KIND>(const Geometry&, dim3, size_t, hipStream_t, const GhmcAdaptMassArgs&);

}  // namespace ghmc_adapt_mass
}  // namespace ebm
