// The H = 128 instantiations of the wide-MLP Euler-Maruyama running-moments kernel -- see mlp_wide_langevin_moments.hip.
#include "mlp_wide_langevin_moments_body.h"

namespace ebm {

int launch_langevin_moments_mlp_wide_h128(const widemlp::WideLangevinMomentsArgs& a, hipStream_t st, const char* who) {
  return widemlp::launch_walk_by_dim<widemlp::LangevinMomentsWalk, 4>(a, st, who);
}

}  // namespace ebm
