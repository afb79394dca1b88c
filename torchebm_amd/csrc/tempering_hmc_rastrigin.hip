// Replica-exchange HMC kernels for one energy (see tempering_hmc_kernel.h); split out so the energies build in parallel.
#include "tempering_hmc_kernel.h"

namespace ebm {
namespace tempering_hmc {
void launch_rastrigin(const rows::Geometry& geo, dim3 grid, size_t smem, hipStream_t st, const TemperHmcArgs& a) {
  launch_kind<EBM_ENERGY_RASTRIGIN>(geo, grid, smem, st, a);
}
}  // namespace tempering_hmc
}  // namespace ebm
