// Annealed-importance-sampling kernels for one energy (see ais_kernel.h); split out so the energies build in parallel.
#include "ais_kernel.h"

namespace ebm {
namespace ais {
void launch_harmonic(const rows::Geometry& geo, dim3 grid, size_t smem, hipStream_t st, const AisArgs& a) {
  launch_kind<EBM_ENERGY_HARMONIC>(geo, grid, smem, st, a);
}
}  // namespace ais
}  // namespace ebm
