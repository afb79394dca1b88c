// The H = 128 instantiations of the wide-MLP annealed-importance-sampling kernel -- see mlp_wide_ais.hip.
#include "mlp_wide_ais_body.h"

namespace ebm {

int launch_ais_mlp_wide_h128(const widemlp::WideAisArgs& a, hipStream_t st, const char* who) {
  return widemlp::launch_walk_by_dim<widemlp::AisWalk, 4>(a, st, who);
}

}  // namespace ebm
