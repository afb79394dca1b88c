// HMC kernels for one energy (see hmc_kernel.h; the energy body: landscape_energies.h); split out so the energies build in parallel.
#include "hmc_kernel.h"
#include "landscape_energies.h"

namespace ebm {
namespace hmc {
void launch_ackley(const rows::Geometry& geo, dim3 grid, size_t smem, hipStream_t st, const HmcArgs& a) {
  launch_kind<EBM_ENERGY_ACKLEY, false>(geo, grid, smem, st, a);
}
}  // namespace hmc
}  // namespace ebm
