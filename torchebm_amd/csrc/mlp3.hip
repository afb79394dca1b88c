// The three-hidden-layer SiLU MLP energy (EBM_ENERGY_MLP3): the two entries of include/ebm_hip_mlp3.h, their refusals, the
// shape table and the H = 64 kernels (mlp3_body.h at HT = 2, DT = 1 / 2 / 4; docs/design/mlp3.md).  The H = 128 kernel is a
// translation unit of its own, mlp3_h128.hip, so that the two compile in parallel.
#include "../../include/ebm_hip_mlp3.h"
#include "mlp3_body.h"

namespace ebm {
namespace mlp3 {
namespace {

// hidden 64 with dim <= 128, or hidden 128 with dim <= 32 (two split 128 x 128 images do not fit LDS; the fp32 words of W1 at
// dim > 32 do not fit beside W2 and W3 either)
int check_shape(const char* who, int32_t hidden, int32_t dim) {
  if (hidden != 64 && hidden != 128) return fail(EBM_EDIM, "%s: hidden width %d (the three-layer kernels take 64 and 128)", who, hidden);
  const int32_t max_dim = hidden == 64 ? 128 : 32;
  if (dim < 1 || dim > max_dim) return fail(EBM_EDIM, "%s: dim %d outside 1 .. %d at hidden width %d", who, dim, max_dim, hidden);
  return 0;
}

int check_energy_mlp3(const char* who, const ebm_energy_t* energy) {
  if (!energy) return fail(EBM_EINVAL, "%s: energy descriptor is NULL", who);
  if (energy->kind != EBM_ENERGY_MLP3) return fail(EBM_EKIND, "%s: this entry takes EBM_ENERGY_MLP3 only (got kind %d)", who, energy->kind);
  if (!energy->dev0) return fail(EBM_EINVAL, "%s: the energy needs the packed parameter pointer", who);
  return 0;
}

int dispatch(const Args& a, int32_t hidden, hipStream_t st, const char* who) {
  if (hidden == 128) return launch_h128(a, st, who);
  if (a.dim <= 32) return launch<2, 1>(a, st, who);
  if (a.dim <= 64) return launch<2, 2>(a, st, who);
  return launch<2, 4>(a, st, who);
}

}  // namespace
}  // namespace mlp3
}  // namespace ebm

using namespace ebm;

extern "C" {

int ebm_energy_grad_mlp3_f32(const ebm_energy_t* energy, const float* x, int64_t n_chains, int32_t dim, float* energy_out,
                             float* grad_out, void* stream) {
  const char* who = "ebm_energy_grad_mlp3_f32";
  if (int r = mlp3::check_energy_mlp3(who, energy)) return r;
  if (!x) return fail(EBM_EINVAL, "%s: state pointer is NULL", who);
  if (n_chains < 0) return fail(EBM_EINVAL, "%s: n_chains < 0", who);
  if (int r = mlp3::check_shape(who, energy->n_comp, dim)) return r;
  if (!aligned16(x) || (grad_out && !aligned16(grad_out))) return fail(EBM_EINVAL, "%s: x / grad_out must be 16-byte aligned", who);
  if (n_chains == 0 || (!energy_out && !grad_out)) return 0;
  mlp3::Args a{};
  a.x_src = x; a.n_chains = n_chains; a.dim = dim; a.k_steps = 0;
  a.params = static_cast<const float*>(energy->dev0);
  a.energy_out = energy_out; a.grad_out = grad_out;
  return mlp3::dispatch(a, energy->n_comp, (hipStream_t)stream, who);
}

int ebm_langevin_chain_mlp3_f32(const ebm_energy_t* energy, const float* x_src, float* x, int64_t n_chains, int32_t dim,
                                int32_t k_steps, float eta, float sqrt_eta, float noise_coef, const float* noise, uint64_t seed,
                                uint64_t offset, void* stream) {
  const char* who = "ebm_langevin_chain_mlp3_f32";
  if (int r = mlp3::check_energy_mlp3(who, energy)) return r;
  if (!x_src || !x) return fail(EBM_EINVAL, "%s: state pointer is NULL", who);
  if (n_chains < 0 || k_steps < 0) return fail(EBM_EINVAL, "%s: n_chains=%lld k_steps=%d", who, (long long)n_chains, k_steps);
  if (int r = mlp3::check_shape(who, energy->n_comp, dim)) return r;
  if (!aligned16(x_src) || !aligned16(x) || (noise && !aligned16(noise)))
    return fail(EBM_EINVAL, "%s: x_src / x / noise must be 16-byte aligned", who);
  const size_t state_bytes = (size_t)n_chains * (size_t)dim * sizeof(float);
  if (x_src != x) {
    const uintptr_t s0 = (uintptr_t)x_src, x0 = (uintptr_t)x;
    if (s0 < x0 + state_bytes && x0 < s0 + state_bytes)
      return fail(EBM_EINVAL, "%s: x_src overlaps x without being x", who);
  }
  const hipStream_t st = (hipStream_t)stream;
  if (n_chains == 0) return 0;
  if (k_steps == 0) {  // no step: the output is the start state
    if (x_src == x) return 0;
    const hipError_t e = hipMemcpyAsync(x, x_src, state_bytes, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) return 0;
    set_error("%s: copying x_src into x failed: %s", who, hipGetErrorString(e));
    return (int)e;
  }
  mlp3::Args a{};
  a.x_src = x_src; a.x = x; a.n_chains = n_chains; a.dim = dim; a.k_steps = k_steps;
  a.eta = eta; a.sqrt_eta = sqrt_eta; a.noise_coef = noise_coef;
  a.noise = noise;
  a.key = RngKey{(uint32_t)seed, (uint32_t)(seed >> 32)};
  a.step0 = offset;
  a.params = static_cast<const float*>(energy->dev0);
  return mlp3::dispatch(a, energy->n_comp, st, who);
}

}  // extern "C"
