// What api.hip hands to mlp3_kinetic.hip for ebm_kinetic_chain_mlp3_f32 (include/ebm_hip_mlp3_kinetic.h): the request of the other
// underdamped-Langevin entries (KineticChainReq, formed by api.hip's kinetic_request) and this energy's launcher.  A header of its
// own beside chain_launch.h, which every kernel unit includes.
#pragma once
#include "chain_launch.h"
#include "../../include/ebm_hip_mlp3_kinetic.h"  // the entry's declaration (a companion of ebm_hip_mlp3.h)

namespace ebm {

// hidden width 64, dim 1 .. 128 (the entry has refused everything else): 32 chains per wave around the split-bf16 evaluation,
// k_steps + 1 of them per call
int kinetic_mlp3_chain_launch(const KineticChainReq&, hipStream_t);

}  // namespace ebm
