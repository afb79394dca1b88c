// The replica-exchange Langevin kernels of ONE energy kind (tempering_kernel.h).  The Makefile compiles this source once per
// kind (-DEBM_UNIT_KIND=...) into tempering_<kind>.o, so that the energies build in parallel.
#include "tempering_kernel.h"

namespace ebm {
namespace tempering {

template <int KIND>
void launch_kind(const Geometry& geo, dim3 grid, size_t smem, hipStream_t st, const TemperArgs& a) {
  EBM_GEO_LAUNCH(tempering_ladder_chain, KIND, geo, grid, dim3(kBlock), smem, st, a);
}
template void launch_kind<EBM_UNIT_KIND>(const Geometry&, dim3, size_t, hipStream_t, const TemperArgs&);

}  // namespace tempering
}  // namespace ebm
