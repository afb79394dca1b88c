// The generalized-HMC kernels of ONE energy kind (ghmc_kernel.h).  The Makefile compiles this source once per kind
// (-DEBM_UNIT_KIND=...) into ghmc_<kind>.o, so that the kinds build in parallel.
#include "ghmc_kernel.h"

namespace ebm {
namespace ghmc {

template <int KIND>
void launch_kind(const Geometry& geo, dim3 grid, size_t smem, hipStream_t st, const GhmcArgs& a) {
  EBM_GEO_LAUNCH_NV1(ghmc_chain, KIND, geo, grid, dim3(kBlock), smem, st, a);  // ghmc.hip refuses wider rows
}
template void launch_kind<EBM_UNIT_KIND>(const Geometry&, dim3, size_t, hipStream_t, const GhmcArgs&);

}  // namespace ghmc
}  // namespace ebm
