// HMC transitions on the three-hidden-layer SiLU MLP energy at hidden width 64: the entry of include/ebm_hip_mlp3_hmc.h, its
// refusals and the three instantiations of mlp3_hmc_body.h's kernel (DT = 1 / 2 / 4 for dim <= 32 / 64 / 128;
// docs/design/mlp3_hmc.md).
#include <cmath>
#include "../../include/ebm_hip_mlp3_hmc.h"
#include "mlp3_hmc_body.h"

using namespace ebm;

extern "C" {

int ebm_hmc_chain_mlp3_f32(const ebm_energy_t* energy, float* x, int64_t n_chains, int32_t dim, int32_t n_mh, int32_t n_leapfrog,
                           float eps, const float* eps_table, int32_t mass_kind, double mass_scalar, int32_t thin, float* traj,
                           uint8_t* accept_mask, uint32_t* accept_count, const float* p_noise, const float* u, uint64_t seed,
                           uint64_t offset, void* stream) {
  const char* who = "ebm_hmc_chain_mlp3_f32";
  if (!energy) return fail(EBM_EINVAL, "%s: energy descriptor is NULL", who);
  if (energy->kind != EBM_ENERGY_MLP3) return fail(EBM_EKIND, "%s: this entry takes EBM_ENERGY_MLP3 only (got kind %d)", who, energy->kind);
  if (!energy->dev0) return fail(EBM_EINVAL, "%s: the energy needs the packed parameter pointer", who);
  if (!x) return fail(EBM_EINVAL, "%s: state pointer is NULL", who);
  if (n_chains < 0 || n_mh < 0 || n_leapfrog < 1 || thin < 1)
    return fail(EBM_EINVAL, "%s: n_chains=%lld n_mh=%d n_leapfrog=%d thin=%d", who, (long long)n_chains, n_mh, n_leapfrog, thin);
  if (energy->n_comp != 64 || dim < 1 || dim > 128)
    return fail(EBM_EDIM, "%s: hidden width %d, dim %d (the transition kernel takes hidden width 64 with dim 1 .. 128)", who,
                energy->n_comp, dim);
  if (mass_kind != EBM_MASS_NONE && mass_kind != EBM_MASS_SCALAR)
    return fail(EBM_EINVAL, "%s: mass kind %d (none or scalar only)", who, mass_kind);
  if (!aligned16(x) || (traj && !aligned16(traj)) || (p_noise && !aligned16(p_noise)))
    return fail(EBM_EINVAL, "%s: x / traj / p_noise must be 16-byte aligned", who);
  if (n_chains == 0 || n_mh == 0) return 0;
  mlp3::HmcArgs a{};
  a.x = x; a.n_chains = n_chains; a.dim = dim; a.n_mh = n_mh; a.n_leapfrog = n_leapfrog;
  a.eps = eps; a.eps_table = eps_table;
  a.mass_kind = mass_kind;
  const double ms = mass_kind == EBM_MASS_SCALAR ? mass_scalar : 1.0;
  a.mass_raw = (float)ms; a.mass_sqrt = (float)sqrt(ms); a.mass_safe = (float)(ms < 1e-10 ? 1e-10 : ms);
  a.thin = thin; a.n_kept = n_mh / thin; a.traj = traj;
  a.accept_mask = accept_mask; a.accept_count = accept_count; a.p_noise = p_noise; a.u = u;
  a.key = RngKey{(uint32_t)seed, (uint32_t)(seed >> 32)};
  a.step0 = offset;
  a.params = static_cast<const float*>(energy->dev0);
  const hipStream_t st = (hipStream_t)stream;
  if (dim <= 32) return mlp3::launch_hmc<1>(a, st, who);
  if (dim <= 64) return mlp3::launch_hmc<2>(a, st, who);
  return mlp3::launch_hmc<4>(a, st, who);
}

}  // extern "C"
