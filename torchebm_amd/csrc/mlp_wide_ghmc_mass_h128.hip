// The H = 128 instantiations of the massed wide-MLP generalized-HMC kernel -- see mlp_wide_ghmc_mass.hip.
#include "mlp_wide_ghmc_mass_body.h"

namespace ebm {

int launch_ghmc_mass_mlp_wide_h128(const widemlp::WideGhmcMassArgs& a, hipStream_t st, const char* who) {
  return widemlp::launch_massed_walk_by_dim<widemlp::GhmcMassWalk, 4>(a, st, who);
}

}  // namespace ebm
