// The H = 128 instantiations of the wide-MLP replica-exchange HMC kernel -- see mlp_wide_tempering.hip.
#include "mlp_wide_tempering_body.h"

namespace ebm {

int launch_tempering_mlp_wide_h128(const widemlp::WideTemperArgs& a, hipStream_t st, const char* who) {
  return widemlp::launch_walk_by_dim<widemlp::TemperWalk, 4>(a, st, who);
}

}  // namespace ebm
