// Entry points of the fused two-hidden-layer SiLU MLP energy
//     E(x) = w3 . silu(W2 silu(W1 x + b1) + b2) + b3,      x in R^dim, dim <= 128, hidden width 64 / 128 / 256
// -- forward AND input-gradient inside the kernel, so the sampler no longer round-trips through autograd (~30 launches)
// every Langevin step.  Every shape runs on the wide kernels (mlp_wide.hip, mlp_wide_hmc.hip).  Rounds 1 and 2 kept a
// kernel of its own for config 5's two-moons network (dim <= 4, H = 128: layer 1 on the VALU, the two H x H contractions
// on the exact-f32 MFMA, two waves per SIMD); on the same box the split-operand bf16 form of the wide kernels takes 0.69 ms
// where it took 0.91 (65 536 chains x 20 steps) and 3.0 ms where it took 4.4 (HMC, L = 10, 10 transitions), so it is gone.
// Reference shape: examples/20-training/01-mcmc-losses/02-persistent-cd/main.py:21-31 (the energy),
// torchebm/samplers/langevin_dynamics.py:154-185 (the loop), core/base_integrator.py:711-731 (the update).
#include "chain_launch.h"

namespace ebm {

namespace {

int mlp_check(const ebm_energy_t& e, int32_t dim, const char* who, bool hmc) {
  if (!e.dev0) return fail(EBM_EINVAL, "%s: packed MLP parameters pointer is NULL", who);
  if (hmc ? !mlp_wide_hmc_supported(e.n_comp, dim) : !mlp_wide_supported(e.n_comp, dim))
    return fail(EBM_EDIM, "%s: the fused MLP energy supports hidden width 64 or 128 (256 in a build made with H256=1) and 1 <= dim <= 128 (got %d, %d)", who,
                e.n_comp, dim);
  return 0;
}

}  // namespace

// Records of the matrix-layout MLP kernels (mlp_wide_body.h): a wave of 32 chains is a "block" of the record geometry.
bool mlp_diag_plan(const ebm_energy_t& e, bool hmc, int64_t n_chains, int32_t dim, diag::DiagArgs& d) {
  if (!e.dev0 || (hmc ? !mlp_wide_hmc_supported(e.n_comp, dim) : !mlp_wide_supported(e.n_comp, dim))) return false;
  return diag::plan(n_chains, dim, 32 * (int64_t)dim, d);
}

int launch_langevin_chain_mlp(const LangevinChainReq& q, hipStream_t st) {
  const char* who = q.rng_dev ? "ebm_langevin_chain_dev_f32" : "ebm_langevin_chain_f32";
  if (int r = mlp_check(q.e, q.dim, who, false)) return r;
  return launch_mlp_wide(q, nullptr, nullptr, st, who);
}

int launch_hmc_chain_mlp(const HmcChainReq& q, hipStream_t st) {
  const char* who = "ebm_hmc_chain_f32";
  if (int r = mlp_check(q.e, q.dim, who, true)) return r;
  return launch_hmc_chain_mlp_wide(q, st, who);
}

int launch_energy_grad_mlp(const ebm_energy_t& e, const float* x, int64_t n_chains, int32_t dim, float* e_out,
                           float* g_out, hipStream_t st) {
  const char* who = "ebm_energy_grad_f32";
  if (int r = mlp_check(e, dim, who, false)) return r;
  // an evaluation is a chain of no steps (k_steps == 0)
  LangevinChainReq q{e, const_cast<float*>(x), n_chains, dim};
  q.thin = 1;
  q.src = q.x;
  return launch_mlp_wide(q, e_out, g_out, st, who);
}

}  // namespace ebm
