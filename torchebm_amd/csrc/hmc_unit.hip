// The lane-group HMC kernels of ONE energy kind (hmc_kernel.h).  The Makefile compiles this source once per kind
// (-DEBM_UNIT_KIND=...) into hmc_<kind>.o, and through hmc_diag_unit.hip into hmc_diag_<kind>.o with the in-kernel
// diagnostics records (hmc_kernel.h: DIAG; diag.h), so that the energies build in parallel.
#include "hmc_kernel.h"
#include "landscape_energies.h"

#ifndef EBM_UNIT_DIAG
#define EBM_UNIT_DIAG false
#endif

namespace ebm {
namespace hmc {

// KERNEL<KIND, G, NV, FULL, MASS, DIAG> over the runtime geometry (see rows.h: EBM_GEO_LAUNCH)
template <int KIND, int MASS, bool DIAG>
void launch_geo(const Geometry& geo, dim3 grid, size_t smem, hipStream_t st, const HmcArgs& a) {
  const dim3 block(kBlock);
#define EBM_HMC_G(GV, NVV, FULLV) hipLaunchKernelGGL((hmc_chain_kernel<KIND, GV, NVV, FULLV, MASS, DIAG>), grid, block, smem, st, a)
  if (geo.NV == 1) {
    switch (geo.G) {
      case 1:  if (geo.full) EBM_HMC_G(1, 1, true);  else EBM_HMC_G(1, 1, false);  break;
      case 2:  if (geo.full) EBM_HMC_G(2, 1, true);  else EBM_HMC_G(2, 1, false);  break;
      case 4:  if (geo.full) EBM_HMC_G(4, 1, true);  else EBM_HMC_G(4, 1, false);  break;
      case 8:  if (geo.full) EBM_HMC_G(8, 1, true);  else EBM_HMC_G(8, 1, false);  break;
      case 16: if (geo.full) EBM_HMC_G(16, 1, true); else EBM_HMC_G(16, 1, false); break;
      case 32: if (geo.full) EBM_HMC_G(32, 1, true); else EBM_HMC_G(32, 1, false); break;
      default: if (geo.full) EBM_HMC_G(64, 1, true); else EBM_HMC_G(64, 1, false); break;
    }
  } else if (geo.NV == 3) {  // element-wise energies, row widths in (2^k, 1.5 2^k] vectors: three vectors per lane (hmc.hip: hmc_geometry)
    if constexpr (KIND == EBM_ENERGY_DOUBLE_WELL || KIND == EBM_ENERGY_HARMONIC) {
      switch (geo.G) {
        case 1:  EBM_HMC_G(1, 3, false);  break;
        case 2:  EBM_HMC_G(2, 3, false);  break;
        case 4:  EBM_HMC_G(4, 3, false);  break;
        case 8:  EBM_HMC_G(8, 3, false);  break;
        case 16: EBM_HMC_G(16, 3, false); break;
        case 32: EBM_HMC_G(32, 3, false); break;
        default: EBM_HMC_G(64, 3, false); break;
      }
    }
  } else if (geo.G == 64 && geo.NV == 2) {
    // (element-wise energies at exactly 512 / 1024 dims: the full-row form -- no per-element masks)
    if constexpr (KIND == EBM_ENERGY_DOUBLE_WELL || KIND == EBM_ENERGY_HARMONIC) {
      if (geo.full) EBM_HMC_G(64, 2, true);
      else EBM_HMC_G(64, 2, false);
    } else {
      EBM_HMC_G(64, 2, false);
    }
  } else if (geo.G == 64 && geo.NV == 4) {
    if constexpr (KIND == EBM_ENERGY_DOUBLE_WELL || KIND == EBM_ENERGY_HARMONIC) {
      if (geo.full) EBM_HMC_G(64, 4, true);
      else EBM_HMC_G(64, 4, false);
    } else {
      EBM_HMC_G(64, 4, false);
    }
  } else if (geo.NV == 4 && geo.full && (geo.G == 4 || geo.G == 8)) {  // element-wise energies at dim 64 / 128
    if constexpr (KIND == EBM_ENERGY_DOUBLE_WELL || KIND == EBM_ENERGY_HARMONIC) {
      if (geo.G == 4) EBM_HMC_G(4, 4, true);
      else EBM_HMC_G(8, 4, true);
    }
  } else if constexpr (KIND >= EBM_ENERGY_ROSENBROCK) {
    // the landscape kinds keep the geometries of pick_geometry: hmc.hip hmc_geometry offers them no dim-32 alternative
  } else if (geo.G == 4 && geo.NV == 2) {  // dim-32 alternatives (full rows only)
    EBM_HMC_G(4, 2, true);
  } else if (geo.G == 2 && geo.NV == 4) {
    EBM_HMC_G(2, 4, true);
  } else if constexpr (KIND == EBM_ENERGY_GMM) {
    // (1, 8) is the small-mixture geometry (K <= 8 at dim 32, hmc.hip: hmc_geometry); with identity mass those calls never get
    // here -- hmc_ring.hip / hmc_gmm32.hip serve them, records included -- so only the massed form is instantiated
    if constexpr (MASS != 0) hipLaunchKernelGGL((hmc_chain_kernel_w2<KIND, 1, 8, true, MASS, DIAG>), grid, block, smem, st, a);
  } else {
    EBM_HMC_G(1, 8, true);
  }
#undef EBM_HMC_G
}

template <int KIND, bool DIAG>
void launch_kind(const Geometry& geo, dim3 grid, size_t smem, hipStream_t st, const HmcArgs& a) {
  if (a.mass_kind == EBM_MASS_NONE) launch_geo<KIND, 0, DIAG>(geo, grid, smem, st, a);
  else launch_geo<KIND, 1, DIAG>(geo, grid, smem, st, a);
}

template void launch_kind<EBM_UNIT_KIND, EBM_UNIT_DIAG>(const Geometry&, dim3, size_t, hipStream_t, const HmcArgs&);

}  // namespace hmc
}  // namespace ebm
