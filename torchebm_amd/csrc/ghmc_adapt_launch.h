// The request of ebm_ghmc_adapt_chain_f32 (include/ebm_hip_adapt.h) and its launcher's declarations: what api.hip hands to
// ghmc_adapt.hip.  A header of its own beside chain_launch.h, which every kernel unit includes.
#pragma once
#include "chain_launch.h"
#include "../../include/ebm_hip_adapt.h"  // the entry's declaration and EBM_DA_* (a companion of ebm_hip.h)

namespace ebm {

struct GhmcAdaptChainReq {
  const ebm_energy_t& e;
  float* x;                // [n_chains, dim], in/out
  float* v;                // [n_chains, dim]: in/out, output only with draw_v0
  int64_t n_chains;
  int32_t dim, n_mh, n_leapfrog;
  // the walk's numbers as they arrived: ghmc_adapt_chain_launch rounds each once to fp32
  double eps0, gamma, temperature, target_accept, mu, eps_min, eps_max;
  int32_t n_adapt, init_da;
  float* da;               // [3, n_chains]
  const float* da_table;   // device [n_adapt, 5]
  bool draw_v0;
  int32_t thin;
  float* traj;             // [n_chains, n_kept(), dim] or null
  uint8_t* accept_mask;    // [n_mh, n_chains] or null
  float* eps_trace;        // [n_mh, n_chains] or null
  float* alpha_mean;       // [n_chains] or null
  const float* noise;      // [n_mh, n_chains, dim] or null
  const float* u;          // [n_mh, n_chains] or null
  uint64_t seed, offset;

  RngKey key() const { return RngKey{(uint32_t)seed, (uint32_t)(seed >> 32)}; }
  int32_t n_kept() const { return n_mh / thin; }
};

// The refusals the adaptation adds to ebm_ghmc_chain_f32's (no launch, no device access): 0, or EBM_EINVAL with the message set
int ghmc_adapt_check(const GhmcAdaptChainReq&, const char* who);
int ghmc_adapt_chain_launch(const GhmcAdaptChainReq&, hipStream_t);

}  // namespace ebm
