// The underdamped-Langevin (BAOAB) kernels of ONE energy kind (kinetic_kernel.h).  The Makefile compiles this source once per
// kind (-DEBM_UNIT_KIND=...) into kinetic_<kind>.o, so that the kinds build in parallel.
#include "kinetic_kernel.h"

namespace ebm {
namespace kinetic {

template <int KIND>
void launch_kind(const Geometry& geo, dim3 grid, size_t smem, hipStream_t st, const KineticArgs& a) {
  EBM_GEO_LAUNCH_NV1(kinetic_chain, KIND, geo, grid, dim3(kBlock), smem, st, a);  // kinetic.hip refuses wider rows
}
template void launch_kind<EBM_UNIT_KIND>(const Geometry&, dim3, size_t, hipStream_t, const KineticArgs&);

}  // namespace kinetic
}  // namespace ebm
