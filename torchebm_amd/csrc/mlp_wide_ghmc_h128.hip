// The H = 128 instantiations of the wide-MLP generalized-HMC kernel -- see mlp_wide_ghmc.hip.
#include "mlp_wide_ghmc_body.h"

namespace ebm {

int launch_ghmc_mlp_wide_h128(const widemlp::WideGhmcArgs& a, hipStream_t st, const char* who) {
  return widemlp::launch_walk_by_dim<widemlp::GhmcWalk, 4>(a, st, who);
}

}  // namespace ebm
