// Replica-exchange Langevin kernels for one energy (see tempering_kernel.h); split out so the energies build in parallel.
#include "tempering_kernel.h"

namespace ebm {
namespace tempering {
void launch_rastrigin(const rows::Geometry& geo, dim3 grid, size_t smem, hipStream_t st, const TemperArgs& a) {
  launch_kind<EBM_ENERGY_RASTRIGIN>(geo, grid, smem, st, a);
}
}  // namespace tempering
}  // namespace ebm
