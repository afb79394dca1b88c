// The H = 128 instantiations of the wide-MLP underdamped-Langevin kernel -- see mlp_wide_kinetic.hip.
#include "mlp_wide_kinetic_body.h"

namespace ebm {

int launch_kinetic_mlp_wide_h128(const widemlp::WideKineticArgs& a, hipStream_t st, const char* who) {
  return widemlp::launch_walk_by_dim<widemlp::KineticWalk, 4>(a, st, who);
}

}  // namespace ebm
