// The H = 128 instantiations of the wide-MLP replica-exchange Langevin kernel -- see mlp_wide_tempering_langevin.hip.
#include "mlp_wide_tempering_langevin_body.h"

namespace ebm {

int launch_tempering_langevin_mlp_wide_h128(const widemlp::WideTemperLangevinArgs& a, hipStream_t st, const char* who) {
  return widemlp::launch_walk_by_dim<widemlp::TemperLangevinWalk, 4>(a, st, who);
}

}  // namespace ebm
