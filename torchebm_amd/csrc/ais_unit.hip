// The annealed-importance-sampling kernels of ONE energy kind (ais_kernel.h).  The Makefile compiles this source once per kind
// (-DEBM_UNIT_KIND=...) into ais_<kind>.o, so that the energies build in parallel.
#include "ais_kernel.h"

namespace ebm {
namespace ais {

template <int KIND>
void launch_kind(const Geometry& geo, dim3 grid, size_t smem, hipStream_t st, const AisArgs& a) {
  EBM_GEO_LAUNCH_NV1(ais_chain, KIND, geo, grid, dim3(kBlock), smem, st, a);  // ais.hip refuses wider rows
}
template void launch_kind<EBM_UNIT_KIND>(const Geometry&, dim3, size_t, hipStream_t, const AisArgs&);

}  // namespace ais
}  // namespace ebm
