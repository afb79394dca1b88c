// The massed underdamped-Langevin kernels of ONE energy kind (kinetic_mass_kernel.h).  The Makefile compiles this source once
// per kind (-DEBM_UNIT_KIND=...) into kinetic_mass_<kind>.o, so that the kinds build in parallel.
#include "kinetic_mass_kernel.h"

namespace ebm {
namespace kinetic_mass {

template <int KIND>
void launch_kind(const Geometry& geo, dim3 grid, size_t smem, hipStream_t st, const KineticMassArgs& a) {
  EBM_GEO_LAUNCH_NV1(kinetic_mass_chain, KIND, geo, grid, dim3(kBlock), smem, st, a);  // kinetic_mass.hip refuses wider rows
}
template void launch_kind<EBM_UNIT_KIND>(const Geometry&, dim3, size_t, hipStream_t, const KineticMassArgs&);

}  // namespace kinetic_mass
}  // namespace ebm
