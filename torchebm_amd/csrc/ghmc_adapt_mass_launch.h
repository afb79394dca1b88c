// The request of ebm_ghmc_adapt_chain_mass_f32 (include/ebm_hip_adapt_mass.h) and its launcher's declaration: what api.hip hands
// to ghmc_adapt_mass.hip -- the unit-mass adapting request (ghmc_adapt_launch.h), whose v is then the momentum plane, and the mass.
#pragma once
#include "ghmc_adapt_launch.h"
#include "../../include/ebm_hip_adapt_mass.h"  // the entry's declaration (a companion of ebm_hip_adapt.h)

namespace ebm {

struct GhmcAdaptMassChainReq {
  GhmcAdaptChainReq chain;
  ChainMass mass;
};

int ghmc_adapt_mass_chain_launch(const GhmcAdaptMassChainReq&, hipStream_t);

}  // namespace ebm
