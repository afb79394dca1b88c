// The H = 128 instantiations of the massed wide-MLP underdamped-Langevin kernel -- see mlp_wide_kinetic_mass.hip.
#include "mlp_wide_kinetic_mass_body.h"

namespace ebm {

int launch_kinetic_mass_mlp_wide_h128(const widemlp::WideKineticMassArgs& a, hipStream_t st, const char* who) {
  return widemlp::launch_massed_walk_by_dim<widemlp::KineticMassWalk, 4>(a, st, who);
}

}  // namespace ebm
