// The H = 128 instantiations of the wide-MLP BAOAB running-moments kernel -- see mlp_wide_kinetic_moments.hip.
#include "mlp_wide_kinetic_moments_body.h"

namespace ebm {

int launch_kinetic_moments_mlp_wide_h128(const widemlp::WideKineticMomentsArgs& a, hipStream_t st, const char* who) {
  return widemlp::launch_walk_by_dim<widemlp::KineticMomentsWalk, 4>(a, st, who);
}

}  // namespace ebm
