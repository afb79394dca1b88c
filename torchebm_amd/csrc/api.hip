// C-ABI entry points of libebm_hip.so (declared in include/ebm_hip.h): argument
// validation, error strings, and dispatch to the kernel launchers.  Nothing here
// allocates device memory or synchronises.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>

#include "chain_launch.h"
#include "../../include/ebm_hip_mass_mlp.h"  // the two massed MLP walks' declarations (a companion of ebm_hip.h)
#include "ghmc_adapt_launch.h"               // the adapting generalized-HMC entry (its companion header: ebm_hip_adapt.h)
#include "ghmc_adapt_mass_launch.h"          // ... with a mass (its companion header: ebm_hip_adapt_mass.h)

namespace ebm {

// launchers implemented in the kernel translation units (the chain launchers: chain_launch.h)
int launch_langevin_step(const float*, const float*, float*, const float*, int64_t, float, float,
                         float, int, float, float, uint64_t, uint64_t, const uint64_t*, hipStream_t);
int launch_langevin_step_diffusion(const float*, const float*, float*, const float*, const float*, int64_t, int64_t, float, float,
                                   uint64_t, uint64_t, hipStream_t);
int launch_diag_finish(const float*, int32_t, int64_t, int32_t, int32_t, int64_t, int32_t, float*, float*, float*, float*,
                       double*, hipStream_t);
int launch_leapfrog_kick_drift(const float*, const float*, const float*, float*, float*, int64_t,
                               int32_t, float, int32_t, double, const float*, int32_t, hipStream_t);
int launch_leapfrog_kick(float*, const float*, const float*, float*, int64_t, float, int32_t,
                         hipStream_t);
int launch_hmc_accept(float*, const float*, const float*, const float*, const float*, uint8_t*,
                      uint32_t*, int64_t, int32_t, uint64_t, uint64_t, const uint64_t*, hipStream_t);
int launch_energy_grad(const ebm_energy_t&, const float*, int64_t, int32_t, float*, float*,
                       hipStream_t);
int launch_chain_stats(const float*, int64_t, int32_t, float*, float*, double*, hipStream_t);
int launch_descent_chain(const ebm_energy_t&, float*, int64_t, int32_t, int32_t, float, const float*, int32_t, float,
                         int32_t, float*, hipStream_t);
int launch_descent_step(const float*, const float*, float*, float*, int64_t, float, float, hipStream_t);
int launch_lookahead(const float*, const float*, float*, int64_t, float, hipStream_t);
int launch_gmm_active_columns(const float*, int32_t, int32_t, int32_t*, hipStream_t);
int launch_pcd_gather(const float*, int64_t, int32_t, float*, int64_t, int64_t, const int64_t*, int64_t*, uint64_t,
                      uint64_t, const uint64_t*, hipStream_t);
int launch_pcd_scatter(float*, int64_t, int32_t, const float*, int64_t, int64_t, const int64_t*, hipStream_t);
int64_t cd_loss_work_bytes();  // misc.hip
int launch_cd_loss(const float*, int64_t, float, void*, float*, float*, hipStream_t);
int launch_cd_loss_seed(const float*, int64_t, float, const float*, const float*, float*, hipStream_t);
int launch_pcd_start_points(const float*, int64_t, int32_t, float*, int64_t, int64_t, int64_t, float, uint64_t, uint64_t, const uint64_t*,
                            hipStream_t);
int launch_noise_fill(float*, int64_t, int32_t, uint64_t, uint64_t, const uint64_t*, hipStream_t);
int launch_energy_grad_mlp(const ebm_energy_t&, const float*, int64_t, int32_t, float*, float*, hipStream_t);
int launch_mlp_backward_acts(int32_t, const float*, const float*, int64_t, int32_t, const float*, float*, float*, float*, hipStream_t, const char*);
int64_t mlp_param_grads_work_floats(int32_t hidden, int32_t dim, int64_t n);  // mlp_param_grads.hip
int launch_mlp_param_grads(int32_t, const float*, const float*, int64_t, int32_t, const float*, const float*, float*, float*, hipStream_t, const char*);
int launch_probe_valu(float*, int32_t, int32_t, hipStream_t);
int launch_probe_issue(float*, int32_t, int32_t, int32_t, hipStream_t);
size_t mlp_w1_image_bytes(int32_t hidden, int32_t dim);  // mlp_wide_slab.hip
int launch_mlp_w1_image(const float* params, int32_t hidden, int32_t dim, void* image, hipStream_t st, const char* who);
size_t gauss_prec_image_bytes(int32_t dim);  // gauss_big_img.hip
int launch_gauss_prec_image(const float* prec, int32_t dim, void* image, hipStream_t st, const char* who);
int launch_energy_grad_gauss_big(const ebm_energy_t&, const float*, int64_t, int32_t, float*, float*, hipStream_t);

namespace {
thread_local char g_err[512] = "";
}

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int check_launch(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return 0;
  set_error("%s: launch failed: %s", what, hipGetErrorString(e));
  return (int)e;
}

namespace {

int check_energy(const ebm_energy_t* en, int32_t dim, const char* who) {
  if (!en) return fail(EBM_EINVAL, "%s: energy descriptor is NULL", who);
  switch (en->kind) {
    case EBM_ENERGY_DOUBLE_WELL:
    case EBM_ENERGY_HARMONIC:
      return 0;
    case EBM_ENERGY_GAUSSIAN:
      if (!en->dev0 || !en->dev1) return fail(EBM_EINVAL, "%s: Gaussian energy needs mean and precision pointers", who);
      return 0;
    case EBM_ENERGY_GMM:
      if (!en->dev0 || !en->dev1 || en->n_comp < 1) return fail(EBM_EINVAL, "%s: mixture energy needs means, log-weights and n_comp >= 1", who);
      if (en->n_comp > 64) return fail(EBM_EDIM, "%s: at most 64 mixture components are supported (got %d)", who, en->n_comp);
      return 0;
    case EBM_ENERGY_MLP:
      if (!en->dev0) return fail(EBM_EINVAL, "%s: MLP energy needs the packed parameter pointer", who);
      return 0;
    case EBM_ENERGY_ROSENBROCK:
      if (dim < 2) return fail(EBM_EDIM, "%s: the Rosenbrock energy needs at least 2 dimensions (got %d)", who, dim);
      return 0;
    case EBM_ENERGY_ACKLEY:
    case EBM_ENERGY_RASTRIGIN:
      return 0;
    default:
      return fail(EBM_EKIND, "%s: unknown energy kind %d", who, en->kind);
  }
  (void)dim;
}

int reject_mlp(const ebm_energy_t* en, const char* who) {
  if (en->kind == EBM_ENERGY_MLP)
    return fail(EBM_EKIND, "%s: the MLP energy is fused for Langevin chains and energy/gradient evaluation only", who);
  return 0;
}

// Which kernel family serves a chain call that asks for diagnostics records, and with what record geometry.
// One function for the layout query and for the dispatch, so the two cannot disagree.
enum DiagFamily { kDiagNone = 0, kDiagElemFlat, kDiagRows, kDiagHmcRows, kDiagMatrix, kDiagMlp, kDiagGaussBig };

DiagFamily plan_diag(const ebm_energy_t& e, int sampler, int64_t n_chains, int32_t dim, bool has_noise, bool has_traj,
                     diag::DiagArgs& d) {
  if (e.kind == EBM_ENERGY_MLP)  // matrix-layout kernels: one record per wave of 32 chains (mlp_wide_body.h); no Heun kernel
    return (sampler != EBM_DIAG_LANGEVIN_HEUN && mlp_diag_plan(e, sampler == EBM_DIAG_HMC, n_chains, dim, d)) ? kDiagMlp : kDiagNone;
  const bool elementwise = e.kind == EBM_ENERGY_DOUBLE_WELL || e.kind == EBM_ENERGY_HARMONIC;
  if (sampler == EBM_DIAG_HMC) return hmc_diag_plan(e, n_chains, dim, d) ? kDiagHmcRows : kDiagNone;
  const int heun = sampler == EBM_DIAG_LANGEVIN_HEUN;
  if (elementwise && elem_diag_supported(dim, has_noise, has_traj) && elem_diag_plan(n_chains, dim, d)) return kDiagElemFlat;
  // dense Gaussians and mixtures where the matrix-layout kernels run (dims up to 96): records from those kernels
  static const bool gauss_rows = ab_switch("EBM_GAUSS_ROWS");
  static const bool gmm_rows = ab_switch("EBM_GMM_ROWS");
  const bool forced_rows = (e.kind == EBM_ENERGY_GAUSSIAN && gauss_rows) || (e.kind == EBM_ENERGY_GMM && gmm_rows);
  if (!heun && !forced_rows && matrix_langevin_diag_plan(e, n_chains, dim, d)) return kDiagMatrix;
  // dense Gaussians above 128 dims: the streamed-Ps kernels (gauss_big.hip) and their records
  if (!heun && !forced_rows && e.kind == EBM_ENERGY_GAUSSIAN && gauss_big_diag_plan(n_chains, dim, d)) return kDiagGaussBig;
  return rows_langevin_diag_plan(e, heun, n_chains, dim, d) ? kDiagRows : kDiagNone;
}

int check_state(const void* x, int64_t n_chains, int32_t dim, const char* who) {
  if (!x) return fail(EBM_EINVAL, "%s: state pointer is NULL", who);
  if (n_chains < 0 || dim < 1) return fail(EBM_EINVAL, "%s: bad shape [%lld, %d]", who, (long long)n_chains, dim);
  if (!aligned16(x)) return fail(EBM_EINVAL, "%s: state pointer must be 16-byte aligned", who);
  return 0;
}

// What the two replica-exchange entries check alike: the energy kind and the slot matrix [n_ladders * n_replicas, dim]
int check_ladders(const ebm_energy_t* energy, const void* x, int64_t n_ladders, int32_t n_replicas, int32_t dim, const char* who) {
  if (energy && energy->kind == EBM_ENERGY_MLP)
    return fail(EBM_EKIND, "%s: the MLP energy has no replica-exchange kernel (the sampler's eager route takes it)", who);
  if (int r = check_energy(energy, dim, who)) return r;
  if (!x) return fail(EBM_EINVAL, "%s: state pointer is NULL", who);
  if (n_replicas < 2 || n_replicas > 64) return fail(EBM_EINVAL, "%s: n_replicas=%d (a ladder has 2 .. 64 slots)", who, n_replicas);
  if (n_ladders < 0 || dim < 1) return fail(EBM_EINVAL, "%s: bad shape [%lld, %d, %d]", who, (long long)n_ladders, n_replicas, dim);
  if (!aligned16(x)) return fail(EBM_EINVAL, "%s: state pointer must be 16-byte aligned", who);
  return 0;
}

// What every entry that walks the MLP energy only checks first: the descriptor, then the kind (`twin` takes the analytic kinds)
int check_mlp_walk(const ebm_energy_t* energy, int32_t dim, const char* who, const char* twin) {
  if (int r = check_energy(energy, dim, who)) return r;
  if (energy->kind != EBM_ENERGY_MLP) return fail(EBM_EKIND, "%s: this entry walks the MLP energy only (%s takes the analytic kinds)", who, twin);
  return 0;
}

// The counted window of the four running-moments entries: two halves of h >= 2 steps behind the burn-in
int check_moments_window(int32_t k_steps, int32_t burn_in, const char* who) {
  if (k_steps < 0 || burn_in < 0 || burn_in > k_steps || ((k_steps - burn_in) & 1) || (k_steps - burn_in) / 2 < 2)
    return fail(EBM_EINVAL, "%s: k_steps=%d burn_in=%d (k_steps - burn_in must be 2 h with h >= 2)", who, k_steps, burn_in);
  return 0;
}

// ebm_langevin_chain_from_f32 on a kernel family that updates in place: the start state goes into the output first
int copy_state(float* x, const float* src, size_t bytes, hipStream_t st, const char* who) {
  const hipError_t e = hipMemcpyAsync(x, src, bytes, hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess) return 0;
  set_error("%s: copying x_src into x failed: %s", who, hipGetErrorString(e));
  return (int)e;
}

}  // namespace
}  // namespace ebm

using namespace ebm;

extern "C" {

int ebm_version(void) { return EBM_ABI_VERSION; }

const char* ebm_last_error_string(void) { return g_err; }

int ebm_langevin_step_f32(const float* x, const float* grad, float* out, const float* noise,
                          int64_t n_elem, float eta, float sqrt_eta, float noise_coef,
                          int32_t clamp_on, float cmin, float cmax, uint64_t seed, uint64_t offset,
                          void* stream) {
  const char* who = "ebm_langevin_step_f32";
  if (n_elem < 0) return fail(EBM_EINVAL, "%s: n_elem < 0", who);
  if (n_elem == 0) return 0;
  if (!x || !out) return fail(EBM_EINVAL, "%s: x/out is NULL", who);
  if (!aligned16(x) || !aligned16(out) || (grad && !aligned16(grad)) || (noise && !aligned16(noise)))
    return fail(EBM_EINVAL, "%s: pointers must be 16-byte aligned", who);
  return launch_langevin_step(x, grad, out, noise, n_elem, eta, sqrt_eta, noise_coef, clamp_on,
                              cmin, cmax, seed, offset, nullptr, (hipStream_t)stream);
}

int ebm_langevin_step_diffusion_f32(const float* x, const float* grad, float* out, const float* noise, const float* diffusion,
                                    int64_t diffusion_period, int64_t n_elem, float eta, float sqrt_eta, uint64_t seed,
                                    uint64_t offset, void* stream) {
  const char* who = "ebm_langevin_step_diffusion_f32";
  if (n_elem < 0) return fail(EBM_EINVAL, "%s: n_elem < 0", who);
  if (n_elem == 0) return 0;
  if (!x || !out || !diffusion) return fail(EBM_EINVAL, "%s: x/out/diffusion is NULL", who);
  if (diffusion_period < 1 || (diffusion_period != 1 && n_elem % diffusion_period != 0))
    return fail(EBM_EINVAL, "%s: diffusion_period %lld does not tile n_elem %lld", who, (long long)diffusion_period, (long long)n_elem);
  if (!aligned16(x) || !aligned16(out) || (grad && !aligned16(grad)) || (noise && !aligned16(noise)))
    return fail(EBM_EINVAL, "%s: pointers must be 16-byte aligned", who);
  return launch_langevin_step_diffusion(x, grad, out, noise, diffusion, diffusion_period, n_elem, eta, sqrt_eta, seed, offset,
                                        (hipStream_t)stream);
}

int ebm_langevin_step_dev_f32(const float* x, const float* grad, float* out, int64_t n_elem, float eta,
                              float sqrt_eta, float noise_coef, int32_t clamp_on, float cmin, float cmax,
                              const uint64_t* rng_state, void* stream) {
  const char* who = "ebm_langevin_step_dev_f32";
  if (n_elem < 0) return fail(EBM_EINVAL, "%s: n_elem < 0", who);
  if (n_elem == 0) return 0;
  if (!x || !out || !rng_state) return fail(EBM_EINVAL, "%s: x/out/rng_state is NULL", who);
  if (!aligned16(x) || !aligned16(out) || (grad && !aligned16(grad)))
    return fail(EBM_EINVAL, "%s: pointers must be 16-byte aligned", who);
  return launch_langevin_step(x, grad, out, nullptr, n_elem, eta, sqrt_eta, noise_coef, clamp_on, cmin, cmax, 0, 0,
                              rng_state, (hipStream_t)stream);
}

// The four Langevin chain entries: validate, decode the flag word, build the request -- once, here -- then route it.
// `dev_rng`: ebm_langevin_chain_dev_f32 (RNG coordinates in device memory, MLP energies only; the MLP kernels never contract,
// so EBM_CHAIN_CONTRACTED is accepted there and ignored).
// `x_src`: ebm_langevin_chain_from_f32's start state (NULL or x itself: the in-place call).  The element-wise kernels load it in
// their prologue and store to x; every other family gets it copied into x here, once, and runs in place as before.
static int langevin_chain_impl(const char* who, int heun, bool dev_rng, const ebm_energy_t* energy, const float* x_src, float* x, int64_t n_chains,
                               int32_t dim, int32_t k_steps, float eta, float sqrt_eta, float noise_coef,
                               const float* coef_table, int32_t clamp_on, float cmin, float cmax, int32_t thin, float* traj,
                               float* diag_partials, const float* noise, uint64_t seed, uint64_t offset,
                               const uint64_t* rng_state, void* stream) {
  if (int r = check_energy(energy, dim, who)) return r;
  if (heun) {
    if (int r = reject_mlp(energy, who)) return r;
  }
  if (int r = check_state(x, n_chains, dim, who)) return r;
  // ABI 8: `clamp_on` is a flag word -- bit 0 the clamp, bit 1 EBM_CHAIN_CONTRACTED (include/ebm_hip.h)
  if (clamp_on & ~(EBM_CHAIN_CLAMP | EBM_CHAIN_CONTRACTED)) return fail(EBM_EINVAL, "%s: unknown bits in clamp_on (%d)", who, clamp_on);
  if (k_steps < 0 || thin < 1) return fail(EBM_EINVAL, "%s: k_steps=%d thin=%d", who, k_steps, thin);
  if (dev_rng) {
    if (!rng_state) return fail(EBM_EINVAL, "%s: rng_state is NULL", who);
    if (energy->kind != EBM_ENERGY_MLP)
      return fail(EBM_EKIND, "%s: device-resident RNG coordinates are taken by the EBM_ENERGY_MLP chain kernels only", who);
  }
  const float* src = x_src ? x_src : x;
  const size_t state_bytes = (size_t)n_chains * (size_t)dim * sizeof(float);
  if (src != x) {
    if (!aligned16(src)) return fail(EBM_EINVAL, "%s: x_src must be 16-byte aligned", who);
    const uintptr_t s0 = (uintptr_t)src, x0 = (uintptr_t)x;
    if (s0 < x0 + state_bytes && x0 < s0 + state_bytes)
      return fail(EBM_EINVAL, "%s: x_src overlaps x without being x (an in-place call passes NULL or x itself)", who);
  }
  const hipStream_t st = (hipStream_t)stream;
  if (n_chains == 0) return 0;
  if (k_steps == 0) {  // no step: the output is the start state
    if (src != x) return copy_state(x, src, state_bytes, st, who);
    return 0;
  }
  if ((coef_table && !aligned16(coef_table)) || (traj && !aligned16(traj)) || (noise && !aligned16(noise)) ||
      (diag_partials && !aligned16(diag_partials)))
    return fail(EBM_EINVAL, "%s: pointers must be 16-byte aligned", who);
  if (k_steps / thin == 0) diag_partials = nullptr;
  const ebm_energy_t& e = *energy;
  diag::DiagArgs d;
  const DiagFamily family =
      diag_partials ? plan_diag(e, heun ? EBM_DIAG_LANGEVIN_HEUN : EBM_DIAG_LANGEVIN, n_chains, dim, noise != nullptr, traj != nullptr, d)
                    : kDiagNone;
  // Who reads the start state from `src`: the element-wise launchers (langevin.hip, langevin_diag.hip).  Every other kernel
  // family updates x in place, so a distinct source is copied into x first and the call goes on as the in-place one.
  const bool elementwise = e.kind == EBM_ENERGY_DOUBLE_WELL || e.kind == EBM_ENERGY_HARMONIC;
  const bool launcher_reads_src = diag_partials ? family == kDiagElemFlat : elementwise;
  const bool no_records = diag_partials && (family == kDiagNone || family == kDiagHmcRows);  // refused below, x left as it is
  if (src != x && !launcher_reads_src && !no_records) {
    if (int r = copy_state(x, src, state_bytes, st, who)) return r;
    src = x;
  }
  const LangevinChainReq q{*energy, x, n_chains, dim, k_steps, eta, sqrt_eta, noise_coef, coef_table,
                           (clamp_on & EBM_CHAIN_CLAMP) != 0, (clamp_on & EBM_CHAIN_CONTRACTED) != 0, cmin, cmax, thin, traj,
                           noise, seed, offset, diag_partials, heun, rng_state, src};
  if (diag_partials) {
    switch (family) {
      case kDiagElemFlat: return launch_langevin_chain_elem_diag(q, st);
      case kDiagRows: return launch_langevin_chain_rows(q, st);
      case kDiagMlp: return launch_langevin_chain_mlp(q, st);
      case kDiagGaussBig: return launch_langevin_chain_gauss_big(q, st);
      case kDiagMatrix: return launch_langevin_chain_matrix_diag(q, st);
      default:
        return fail(e.kind == EBM_ENERGY_MLP ? EBM_EKIND : EBM_EDIM,
                    "%s: no in-kernel diagnostics for this energy / dim %d (see ebm_diag_layout)", who, dim);
    }
  }
  if (e.kind == EBM_ENERGY_MLP) return launch_langevin_chain_mlp(q, st);
  if (e.kind == EBM_ENERGY_DOUBLE_WELL || e.kind == EBM_ENERGY_HARMONIC) return launch_langevin_chain_elem(q, st);
  if (!heun && e.kind == EBM_ENERGY_GAUSSIAN && gauss_shift_supported(dim)) {
    // A/B switch: EBM_GAUSS_NOSHIFT=1 keeps the packed rows / the lane-group kernel for widths off multiples of 4
    static const bool no_shift = ab_switch("EBM_GAUSS_NOSHIFT");
    if (!no_shift) return launch_langevin_chain_gauss_shift(q, st);
  }
  if (!heun && gauss_res_shift_supported(e, dim)) {
    static const bool no_shift = ab_switch("EBM_GAUSS_NOSHIFT");
    if (!no_shift) return launch_langevin_chain_gauss_res_shift(q, st);
  }
  if (!heun && e.kind == EBM_ENERGY_GAUSSIAN && gauss_pack_factor(dim, n_chains) >= 1) {
    // A/B switch for tests and profiling: EBM_GAUSS_ROWS=1 keeps the LDS mat-vec kernel
    static const bool force_rows = ab_switch("EBM_GAUSS_ROWS");
    if (!force_rows) return launch_langevin_chain_gauss_mfma(q, st);
  }
  if (!heun && e.kind == EBM_ENERGY_GAUSSIAN && gauss_lds5_supported(dim)) {
    static const bool force_big = ab_switch("EBM_GAUSS_NO_LDS5");
    if (!force_big) return launch_langevin_chain_gauss_mfma(q, st);
  }
  if (!heun && e.kind == EBM_ENERGY_GAUSSIAN && gauss_big_supported(dim)) {
    static const bool force_rows = ab_switch("EBM_GAUSS_ROWS");
    if (!force_rows) return launch_langevin_chain_gauss_big(q, st);
  }
  if (!heun && e.kind == EBM_ENERGY_GMM && (gmm_wide_supported(dim, e.n_comp) || gmm_wide_shift_supported(dim, e.n_comp))) {
    static const bool no_wide = ab_switch("EBM_GMM_NOWIDE");  // A/B switch: the lane-group kernels above 128 dims
    if (!no_wide)
      return gmm_wide_supported(dim, e.n_comp) ? launch_langevin_chain_gmm_wide(q, st) : launch_langevin_chain_gmm_wide_shift(q, st);
  }
  if (!heun && e.kind == EBM_ENERGY_GMM && gmm_shift_supported(dim, e.n_comp)) {
    static const bool no_shift = ab_switch("EBM_GAUSS_NOSHIFT");
    if (!no_shift) return launch_langevin_chain_gmm_shift(q, st);
  }
  // mixtures of up to 32 components on the matrix layout (gauss_mfma.hip / gmm_bf16x3.h); dims 16 / 32 with K <= 8 keep
  // one lane per chain with the means as scalar operands
  if (!heun && e.kind == EBM_ENERGY_GMM && gmm_mfma_supported(dim, e.n_comp) && !(dim == 32 && e.n_comp <= 8)) {
    static const bool force_rows = ab_switch("EBM_GMM_ROWS");
    if (!force_rows) return launch_langevin_chain_gmm_mfma(q, st);
  }
  return launch_langevin_chain_rows(q, st);
}

int ebm_langevin_chain_f32(const ebm_energy_t* energy, float* x, int64_t n_chains, int32_t dim,
                           int32_t k_steps, float eta, float sqrt_eta, float noise_coef,
                           const float* coef_table, int32_t clamp_on, float cmin, float cmax,
                           int32_t thin, float* traj, float* diag_partials, const float* noise, uint64_t seed,
                           uint64_t offset, void* stream) {
  return langevin_chain_impl("ebm_langevin_chain_f32", 0, false, energy, nullptr, x, n_chains, dim, k_steps, eta, sqrt_eta, noise_coef,
                             coef_table, clamp_on, cmin, cmax, thin, traj, diag_partials, noise, seed, offset, nullptr, stream);
}

int ebm_langevin_chain_from_f32(const ebm_energy_t* energy, const float* x_src, float* x, int64_t n_chains, int32_t dim,
                                int32_t k_steps, float eta, float sqrt_eta, float noise_coef,
                                const float* coef_table, int32_t clamp_on, float cmin, float cmax,
                                int32_t thin, float* traj, float* diag_partials, const float* noise, uint64_t seed,
                                uint64_t offset, void* stream) {
  return langevin_chain_impl("ebm_langevin_chain_from_f32", 0, false, energy, x_src, x, n_chains, dim, k_steps, eta, sqrt_eta,
                             noise_coef, coef_table, clamp_on, cmin, cmax, thin, traj, diag_partials, noise, seed, offset, nullptr,
                             stream);
}

int ebm_langevin_chain_dev_f32(const ebm_energy_t* energy, float* x, int64_t n_chains, int32_t dim, int32_t k_steps,
                               float eta, float sqrt_eta, float noise_coef, const float* coef_table, int32_t clamp_on,
                               float cmin, float cmax, int32_t thin, float* traj, const uint64_t* rng_state,
                               uint64_t step_delta, void* stream) {
  return langevin_chain_impl("ebm_langevin_chain_dev_f32", 0, true, energy, nullptr, x, n_chains, dim, k_steps, eta, sqrt_eta, noise_coef,
                             coef_table, clamp_on, cmin, cmax, thin, traj, nullptr, nullptr, 0, step_delta, rng_state, stream);
}

int ebm_langevin_heun_chain_f32(const ebm_energy_t* energy, float* x, int64_t n_chains, int32_t dim,
                                int32_t k_steps, float eta, float sqrt_eta, float noise_coef,
                                const float* coef_table, int32_t clamp_on, float cmin, float cmax,
                                int32_t thin, float* traj, float* diag_partials, const float* noise, uint64_t seed,
                                uint64_t offset, void* stream) {
  return langevin_chain_impl("ebm_langevin_heun_chain_f32", 1, false, energy, nullptr, x, n_chains, dim, k_steps, eta, sqrt_eta, noise_coef,
                             coef_table, clamp_on, cmin, cmax, thin, traj, diag_partials, noise, seed, offset, nullptr, stream);
}

// The two HMC chain entries: validate and build the request once, then route it.
static int hmc_chain_impl(const char* who, bool audit, const ebm_energy_t* energy, float* x, int64_t n_chains, int32_t dim,
                          int32_t n_mh, int32_t n_leapfrog, float eps, const float* eps_table, int32_t mass_kind, double mass_scalar,
                          const float* mass_diag, int32_t thin, float* traj, float* diag_partials, uint8_t* accept_mask,
                          uint32_t* accept_count, const float* p_noise, const float* u, uint64_t seed, uint64_t offset,
                          void* stream) {
  if (int r = check_energy(energy, dim, who)) return r;
  if (int r = check_state(x, n_chains, dim, who)) return r;
  if (n_mh < 0 || thin < 1 || n_leapfrog < 1)
    return fail(EBM_EINVAL, "%s: n_mh=%d thin=%d n_leapfrog=%d", who, n_mh, thin, n_leapfrog);
  if (mass_kind < EBM_MASS_NONE || mass_kind > EBM_MASS_DIAG || (mass_kind == EBM_MASS_DIAG && !mass_diag))
    return fail(EBM_EINVAL, "%s: bad mass specification (kind %d)", who, mass_kind);
  if ((p_noise == nullptr) != (u == nullptr))
    return fail(EBM_EINVAL, "%s: p_noise and u must be given together", who);
  if (n_chains == 0 || n_mh == 0) return 0;
  if ((traj && !aligned16(traj)) || (p_noise && !aligned16(p_noise)) || (diag_partials && !aligned16(diag_partials)))
    return fail(EBM_EINVAL, "%s: pointers must be 16-byte aligned", who);
  if (n_mh / thin == 0) diag_partials = nullptr;
  const HmcChainReq q{*energy, x, n_chains, dim, n_mh, n_leapfrog, eps, eps_table, mass_kind, mass_scalar, mass_diag, thin, traj,
                      accept_mask, accept_count, p_noise, u, seed, offset, diag_partials};
  const hipStream_t st = (hipStream_t)stream;
  if (audit) return launch_hmc_chain_audit(q, st);
  if (diag_partials) {
    diag::DiagArgs d;
    const DiagFamily fam = plan_diag(*energy, EBM_DIAG_HMC, n_chains, dim, p_noise != nullptr, traj != nullptr, d);
    if (fam != kDiagHmcRows && fam != kDiagMlp)
      return fail(energy->kind == EBM_ENERGY_MLP ? EBM_EKIND : EBM_EDIM,
                  "%s: no in-kernel diagnostics for this energy / dim %d (see ebm_diag_layout)", who, dim);
  }
  if (energy->kind == EBM_ENERGY_MLP) return launch_hmc_chain_mlp(q, st);
  return launch_hmc_chain(q, st);
}

int ebm_hmc_chain_f32(const ebm_energy_t* energy, float* x, int64_t n_chains, int32_t dim,
                      int32_t n_mh, int32_t n_leapfrog, float eps, const float* eps_table,
                      int32_t mass_kind, double mass_scalar, const float* mass_diag, int32_t thin,
                      float* traj, float* diag_partials, uint8_t* accept_mask, uint32_t* accept_count,
                      const float* p_noise, const float* u, uint64_t seed, uint64_t offset,
                      void* stream) {
  return hmc_chain_impl("ebm_hmc_chain_f32", false, energy, x, n_chains, dim, n_mh, n_leapfrog, eps, eps_table, mass_kind, mass_scalar,
                        mass_diag, thin, traj, diag_partials, accept_mask, accept_count, p_noise, u, seed, offset, stream);
}

int ebm_hmc_chain_audit_f32(const ebm_energy_t* energy, float* x, int64_t n_chains, int32_t dim, int32_t n_mh, int32_t n_leapfrog,
                            float eps, const float* eps_table, int32_t mass_kind, double mass_scalar, const float* mass_diag,
                            int32_t thin, float* traj, uint8_t* accept_mask, uint32_t* accept_count, const float* p_noise,
                            const float* u, uint64_t seed, uint64_t offset, void* stream) {
  return hmc_chain_impl("ebm_hmc_chain_audit_f32", true, energy, x, n_chains, dim, n_mh, n_leapfrog, eps, eps_table, mass_kind,
                        mass_scalar, mass_diag, thin, traj, nullptr, accept_mask, accept_count, p_noise, u, seed, offset, stream);
}

int ebm_tempering_chain_f32(const ebm_energy_t* energy, float* x, int64_t n_ladders, int32_t n_replicas, int32_t dim,
                            int32_t k_steps, float eta, float sqrt_eta, const float* noise_coef, const float* beta,
                            int32_t swap_every, int32_t thin, float* traj, uint32_t* swap_counts, const float* noise,
                            const float* u, uint64_t seed, uint64_t step0, void* stream) {
  const char* who = "ebm_tempering_chain_f32";
  if (int r = check_ladders(energy, x, n_ladders, n_replicas, dim, who)) return r;
  if (k_steps < 0 || swap_every < 1 || thin < 1)
    return fail(EBM_EINVAL, "%s: k_steps=%d swap_every=%d thin=%d", who, k_steps, swap_every, thin);
  if (int r = tempering_check_geometry(n_replicas, dim)) return r;
  if (!noise_coef || !beta) return fail(EBM_EINVAL, "%s: noise_coef / beta is NULL", who);
  if ((noise == nullptr) != (u == nullptr)) return fail(EBM_EINVAL, "%s: noise and u must be given together", who);
  if (n_ladders == 0 || k_steps == 0) return 0;
  if ((traj && !aligned16(traj)) || (noise && !aligned16(noise))) return fail(EBM_EINVAL, "%s: pointers must be 16-byte aligned", who);
  const TemperingChainReq q{*energy, x, n_ladders, n_replicas, dim, k_steps, eta, sqrt_eta, noise_coef, beta, swap_every, thin,
                            traj, swap_counts, noise, u, seed, step0};
  return tempering_chain_launch(q, (hipStream_t)stream);
}

int ebm_tempering_mlp_chain_f32(const ebm_energy_t* energy, float* x, int64_t n_ladders, int32_t n_replicas, int32_t dim,
                                int32_t k_steps, float eta, float sqrt_eta, const float* noise_coef, const float* beta,
                                int32_t swap_every, int32_t thin, float* traj, uint32_t* swap_counts, const float* noise,
                                const float* u, uint64_t seed, uint64_t step0, void* stream) {
  const char* who = "ebm_tempering_mlp_chain_f32";
  if (int r = check_mlp_walk(energy, dim, who, "ebm_tempering_chain_f32")) return r;
  // (the dim range and the ladder lengths are wide_mlp_check_ladder_shape's to refuse)
  if (!x) return fail(EBM_EINVAL, "%s: state pointer is NULL", who);
  if (!noise_coef || !beta) return fail(EBM_EINVAL, "%s: noise_coef / beta is NULL", who);
  if (n_ladders < 0) return fail(EBM_EINVAL, "%s: bad shape [%lld, %d, %d]", who, (long long)n_ladders, n_replicas, dim);
  if (k_steps < 1 || swap_every < 1 || thin < 1)
    return fail(EBM_EINVAL, "%s: k_steps=%d swap_every=%d thin=%d (all must be >= 1)", who, k_steps, swap_every, thin);
  if ((noise == nullptr) != (u == nullptr)) return fail(EBM_EINVAL, "%s: noise and u must be given together", who);
  if (!std::isfinite(eta) || !std::isfinite(sqrt_eta))
    return fail(EBM_EINVAL, "%s: eta=%g sqrt_eta=%g (both must be finite)", who, (double)eta, (double)sqrt_eta);
  if (!aligned16(x) || (traj && !aligned16(traj)) || (noise && !aligned16(noise)))
    return fail(EBM_EINVAL, "%s: pointers must be 16-byte aligned", who);
  if (int r = wide_mlp_check_ladder_shape(who, energy->n_comp, dim, n_replicas)) return r;
  if (n_ladders == 0) return 0;
  const TemperingChainReq q{*energy, x, n_ladders, n_replicas, dim, k_steps, eta, sqrt_eta, noise_coef, beta, swap_every, thin,
                            traj, swap_counts, noise, u, seed, step0};
  return tempering_mlp_chain_launch(q, (hipStream_t)stream);
}

int ebm_tempering_hmc_chain_f32(const ebm_energy_t* energy, float* x, int64_t n_ladders, int32_t n_replicas, int32_t dim,
                                int32_t n_mh, int32_t n_leapfrog, const float* eps, const float* sqrt_temp, const float* beta,
                                int32_t swap_every, int32_t thin, float* traj, uint8_t* accept_mask, uint32_t* accept_counts,
                                uint32_t* swap_counts, const float* p_noise, const float* u_accept, const float* u_swap,
                                uint64_t seed, uint64_t step0, void* stream) {
  const char* who = "ebm_tempering_hmc_chain_f32";
  if (int r = check_ladders(energy, x, n_ladders, n_replicas, dim, who)) return r;
  if (n_mh < 0 || n_leapfrog < 1 || swap_every < 1 || thin < 1)
    return fail(EBM_EINVAL, "%s: n_mh=%d n_leapfrog=%d swap_every=%d thin=%d", who, n_mh, n_leapfrog, swap_every, thin);
  if (int r = tempering_hmc_check_geometry(n_replicas, dim)) return r;
  if (!eps || !sqrt_temp || !beta) return fail(EBM_EINVAL, "%s: eps / sqrt_temp / beta is NULL", who);
  if ((p_noise == nullptr) != (u_accept == nullptr) || (p_noise == nullptr) != (u_swap == nullptr))
    return fail(EBM_EINVAL, "%s: p_noise, u_accept and u_swap must be given together", who);
  if (n_ladders == 0 || n_mh == 0) return 0;
  if ((traj && !aligned16(traj)) || (p_noise && !aligned16(p_noise))) return fail(EBM_EINVAL, "%s: pointers must be 16-byte aligned", who);
  const TemperingHmcChainReq q{*energy, x, n_ladders, n_replicas, dim, n_mh, n_leapfrog, eps, sqrt_temp, beta, swap_every, thin,
                               traj, accept_mask, accept_counts, swap_counts, p_noise, u_accept, u_swap, seed, step0};
  return tempering_hmc_chain_launch(q, (hipStream_t)stream);
}

int ebm_tempering_hmc_mlp_chain_f32(const ebm_energy_t* energy, float* x, int64_t n_ladders, int32_t n_replicas, int32_t dim,
                                    int32_t n_mh, int32_t n_leapfrog, const float* eps, const float* sqrt_temp, const float* beta,
                                    int32_t swap_every, int32_t thin, float* traj, uint8_t* accept_mask, uint32_t* accept_counts,
                                    uint32_t* swap_counts, const float* p_noise, const float* u_accept, const float* u_swap,
                                    uint64_t seed, uint64_t step0, void* stream) {
  const char* who = "ebm_tempering_hmc_mlp_chain_f32";
  if (int r = check_mlp_walk(energy, dim, who, "ebm_tempering_hmc_chain_f32")) return r;
  // (the dim range and the ladder lengths are wide_mlp_check_ladder_shape's to refuse)
  if (!x) return fail(EBM_EINVAL, "%s: state pointer is NULL", who);
  if (!eps || !sqrt_temp || !beta) return fail(EBM_EINVAL, "%s: eps / sqrt_temp / beta is NULL", who);
  if (n_ladders < 0) return fail(EBM_EINVAL, "%s: bad shape [%lld, %d, %d]", who, (long long)n_ladders, n_replicas, dim);
  if (n_mh < 1 || n_leapfrog < 1 || swap_every < 1 || thin < 1)
    return fail(EBM_EINVAL, "%s: n_mh=%d n_leapfrog=%d swap_every=%d thin=%d (all must be >= 1)", who, n_mh, n_leapfrog, swap_every,
                thin);
  if ((p_noise == nullptr) != (u_accept == nullptr) || (p_noise == nullptr) != (u_swap == nullptr))
    return fail(EBM_EINVAL, "%s: p_noise, u_accept and u_swap must be given together", who);
  if (!aligned16(x) || (traj && !aligned16(traj)) || (p_noise && !aligned16(p_noise)))
    return fail(EBM_EINVAL, "%s: pointers must be 16-byte aligned", who);
  if (int r = wide_mlp_check_ladder_shape(who, energy->n_comp, dim, n_replicas)) return r;
  if (n_ladders == 0) return 0;
  const TemperingHmcChainReq q{*energy, x, n_ladders, n_replicas, dim, n_mh, n_leapfrog, eps, sqrt_temp, beta, swap_every, thin,
                               traj, accept_mask, accept_counts, swap_counts, p_noise, u_accept, u_swap, seed, step0};
  return tempering_hmc_mlp_chain_launch(q, (hipStream_t)stream);
}

// Both annealed-importance-sampling entries: the analytic kinds on the lane-group kernel, the MLP energy on the matrix cores
static int ais_chain_impl(const char* who, bool mlp, const ebm_energy_t* energy, float* x, float* logw, int64_t n_chains, int32_t dim,
                          int32_t n_temps, int32_t n_leapfrog, const float* beta, const float* eps, float sigma0, float inv_var0,
                          uint8_t* accept_mask, uint32_t* accept_counts, const float* x0, const float* p_noise, const float* u_accept,
                          uint64_t seed, uint64_t step0, void* stream) {
  if (!mlp && energy && energy->kind == EBM_ENERGY_MLP)
    return fail(EBM_EKIND, "%s: the MLP energy has no annealed-importance-sampling kernel (the sampler's eager route takes it)", who);
  if (int r = mlp ? check_mlp_walk(energy, dim, who, "ebm_ais_chain_f32") : check_energy(energy, dim, who)) return r;
  if (!x) return fail(EBM_EINVAL, "%s: state pointer is NULL", who);
  // (the MLP walk's dim range is wide_mlp_check_shape's to refuse)
  if (n_chains < 0 || (!mlp && dim < 1)) return fail(EBM_EINVAL, "%s: bad shape [%lld, %d]", who, (long long)n_chains, dim);
  if (!aligned16(x)) return fail(EBM_EINVAL, "%s: state pointer must be 16-byte aligned", who);
  if (!logw) return fail(EBM_EINVAL, "%s: logw is NULL", who);
  if (n_temps < 1 || n_leapfrog < 1) return fail(EBM_EINVAL, "%s: n_temps=%d n_leapfrog=%d", who, n_temps, n_leapfrog);
  if (!mlp)
    if (int r = ais_check_geometry(dim)) return r;
  if (!beta || !eps) return fail(EBM_EINVAL, "%s: beta / eps is NULL", who);
  if ((x0 == nullptr) != (p_noise == nullptr) || (x0 == nullptr) != (u_accept == nullptr))
    return fail(EBM_EINVAL, "%s: x0, p_noise and u_accept must be given together", who);
  if (mlp)
    if (int r = wide_mlp_check_shape(who, energy->n_comp, dim)) return r;
  if (n_chains == 0) return 0;
  if ((x0 && !aligned16(x0)) || (p_noise && !aligned16(p_noise))) return fail(EBM_EINVAL, "%s: pointers must be 16-byte aligned", who);
  const AisChainReq q{*energy, x, logw, n_chains, dim, n_temps, n_leapfrog, beta, eps, sigma0, inv_var0, accept_mask, accept_counts,
                      x0, p_noise, u_accept, seed, step0};
  return mlp ? ais_mlp_chain_launch(q, (hipStream_t)stream) : ais_chain_launch(q, (hipStream_t)stream);
}

int ebm_ais_chain_f32(const ebm_energy_t* energy, float* x, float* logw, int64_t n_chains, int32_t dim, int32_t n_temps,
                      int32_t n_leapfrog, const float* beta, const float* eps, float sigma0, float inv_var0, uint8_t* accept_mask,
                      uint32_t* accept_counts, const float* x0, const float* p_noise, const float* u_accept, uint64_t seed,
                      uint64_t step0, void* stream) {
  return ais_chain_impl("ebm_ais_chain_f32", false, energy, x, logw, n_chains, dim, n_temps, n_leapfrog, beta, eps, sigma0, inv_var0,
                        accept_mask, accept_counts, x0, p_noise, u_accept, seed, step0, stream);
}

int ebm_ais_mlp_chain_f32(const ebm_energy_t* energy, float* x, float* logw, int64_t n_chains, int32_t dim, int32_t n_temps,
                          int32_t n_leapfrog, const float* beta, const float* eps, float sigma0, float inv_var0, uint8_t* accept_mask,
                          uint32_t* accept_counts, const float* x0, const float* p_noise, const float* u_accept, uint64_t seed,
                          uint64_t step0, void* stream) {
  return ais_chain_impl("ebm_ais_mlp_chain_f32", true, energy, x, logw, n_chains, dim, n_temps, n_leapfrog, beta, eps, sigma0, inv_var0,
                        accept_mask, accept_counts, x0, p_noise, u_accept, seed, step0, stream);
}

int ebm_chain_moments_f32(const ebm_energy_t* energy, float* x, int64_t n_chains, int32_t dim, int32_t sampler, int32_t k_steps,
                          int32_t burn_in, float eta, float sqrt_eta, float noise_coef, int32_t n_leapfrog, float eps,
                          const float* recip, float* mom, float* e_mom, float* traj, float* e_traj, uint8_t* accept_mask,
                          uint32_t* accept_count, const float* noise_or_p, const float* u, uint64_t seed, uint64_t offset,
                          void* stream) {
  const char* who = "ebm_chain_moments_f32";
  if (energy && energy->kind == EBM_ENERGY_MLP)
    return fail(EBM_EKIND, "%s: the MLP energy has no running-moments kernel (the samplers' eager route takes it)", who);
  if (int r = check_energy(energy, dim, who)) return r;
  if (int r = check_state(x, n_chains, dim, who)) return r;
  if (sampler != 0 && sampler != 1) return fail(EBM_EINVAL, "%s: sampler=%d (0 = Langevin, 1 = HMC)", who, sampler);
  const bool hmc = sampler == 1;
  if (int r = check_moments_window(k_steps, burn_in, who)) return r;
  if (hmc && n_leapfrog < 1) return fail(EBM_EINVAL, "%s: n_leapfrog=%d", who, n_leapfrog);
  if (int r = moments_check_geometry(dim)) return r;
  if (!recip || !mom) return fail(EBM_EINVAL, "%s: recip / mom is NULL", who);
  if (hmc && (noise_or_p == nullptr) != (u == nullptr)) return fail(EBM_EINVAL, "%s: p_noise and u must be given together", who);
  if (n_chains == 0) return 0;
  if (!aligned16(mom) || (traj && !aligned16(traj)) || (noise_or_p && !aligned16(noise_or_p)))
    return fail(EBM_EINVAL, "%s: pointers must be 16-byte aligned", who);
  const MomentsChainReq q{*energy, x, n_chains, dim, hmc, k_steps, burn_in, eta, sqrt_eta, noise_coef, n_leapfrog, eps, recip, mom,
                          e_mom, traj, e_traj, hmc ? accept_mask : nullptr, hmc ? accept_count : nullptr, noise_or_p,
                          hmc ? u : nullptr, seed, offset};
  return moments_chain_launch(q, (hipStream_t)stream);
}

int ebm_chain_moments_mlp_f32(const ebm_energy_t* energy, float* x, int64_t n_chains, int32_t dim, int32_t sampler, int32_t k_steps,
                              int32_t burn_in, float eta, float sqrt_eta, float noise_coef, int32_t n_leapfrog, float eps,
                              const float* recip, float* mom, float* e_mom, float* traj, float* e_traj, uint8_t* accept_mask,
                              uint32_t* accept_count, const float* noise, const float* u, uint64_t seed, uint64_t offset,
                              void* stream) {
  const char* who = "ebm_chain_moments_mlp_f32";
  (void)n_leapfrog; (void)eps; (void)accept_mask; (void)accept_count; (void)u;  // the HMC half of the shared parameter list
  if (int r = check_mlp_walk(energy, dim, who, "ebm_chain_moments_f32")) return r;
  // (the dim range is wide_mlp_check_shape's to refuse)
  if (!x) return fail(EBM_EINVAL, "%s: state pointer is NULL", who);
  if (n_chains < 0) return fail(EBM_EINVAL, "%s: bad shape [%lld, %d]", who, (long long)n_chains, dim);
  if (sampler != 0)
    return fail(EBM_EINVAL, "%s: sampler=%d (0 = Langevin; for HMC on the MLP: ebm_kinetic_moments_mlp_f32, generalized HMC at infinite friction)",
                who, sampler);
  if (int r = check_moments_window(k_steps, burn_in, who)) return r;
  if (!std::isfinite(eta) || !std::isfinite(sqrt_eta) || !std::isfinite(noise_coef))
    return fail(EBM_EINVAL, "%s: eta=%g sqrt_eta=%g noise_coef=%g (all must be finite)", who, (double)eta, (double)sqrt_eta,
                (double)noise_coef);
  if (!recip || !mom) return fail(EBM_EINVAL, "%s: recip / mom is NULL", who);
  if (int r = wide_mlp_check_shape(who, energy->n_comp, dim)) return r;
  if (n_chains == 0) return 0;
  if (!aligned16(x) || !aligned16(mom) || (traj && !aligned16(traj)) || (noise && !aligned16(noise)))
    return fail(EBM_EINVAL, "%s: pointers must be 16-byte aligned", who);
  const LangevinMomentsChainReq q{*energy, x, n_chains, dim, k_steps, burn_in, eta, sqrt_eta, noise_coef, recip, mom, e_mom, traj,
                                  e_traj, noise, seed, offset};
  return langevin_moments_mlp_chain_launch(q, (hipStream_t)stream);
}

// What the massed entries ask of their mass (the forms of ebm_hmc_chain_f32; EBM_MASS_NONE belongs to the unit-mass entries)
static int check_chain_mass(const ChainMass& m, const char* who) {
  if (m.kind != EBM_MASS_SCALAR && m.kind != EBM_MASS_DIAG)
    return fail(EBM_EINVAL, "%s: mass_kind=%d (EBM_MASS_SCALAR or EBM_MASS_DIAG; the unit-mass entry takes no mass)", who, m.kind);
  if (m.kind == EBM_MASS_DIAG && !m.diag) return fail(EBM_EINVAL, "%s: mass_diag is NULL", who);
  if (m.kind == EBM_MASS_SCALAR && (!(m.scalar > 0.0) || !std::isfinite(m.scalar)))
    return fail(EBM_EINVAL, "%s: mass_scalar=%g (must be positive and finite)", who, m.scalar);
  return 0;
}

// The request of both underdamped-Langevin entries: the constants of the splitting, formed in double, each rounded once
static KineticChainReq kinetic_request(const ebm_energy_t* energy, float* x, float* v, int64_t n_chains, int32_t dim, int32_t k_steps,
                                       double h, double gamma, double temperature, int32_t draw_v0, int32_t thin, float* traj,
                                       const float* noise, uint64_t seed, uint64_t offset) {
  const float hh = (float)(0.5 * h);
  const float c1 = (float)exp(-gamma * h);
  const float c2 = (float)sqrt(temperature * (-expm1(-2.0 * gamma * h)));
  const float sqrt_temp = (float)sqrt(temperature);
  return KineticChainReq{*energy, x, v, n_chains, dim, k_steps, hh, c1, c2, sqrt_temp, draw_v0 != 0, thin, traj, noise, seed, offset};
}

// Both underdamped-Langevin entries: the analytic kinds on the lane-group kernel, the MLP energy on the matrix cores.  The analytic
// entry refuses dim < 1 and a misaligned x with its state; the MLP entry leaves the dim range to wide_mlp_check_shape and checks
// every pointer's alignment behind the empty call.
static int kinetic_chain_impl(const char* who, bool mlp, const ebm_energy_t* energy, float* x, float* v, int64_t n_chains, int32_t dim,
                              int32_t k_steps, double h, double gamma, double temperature, int32_t draw_v0, int32_t thin, float* traj,
                              const float* noise, uint64_t seed, uint64_t offset, void* stream, const ChainMass* mass = nullptr) {
  if (!mlp && energy && energy->kind == EBM_ENERGY_MLP)
    return fail(EBM_EKIND, "%s: the MLP energy has no underdamped-Langevin kernel (the sampler's eager route takes it)", who);
  if (int r = mlp ? check_mlp_walk(energy, dim, who, mass ? "ebm_kinetic_chain_mass_f32" : "ebm_kinetic_chain_f32")
                  : check_energy(energy, dim, who))
    return r;
  if (!mlp) {
    if (int r = check_state(x, n_chains, dim, who)) return r;
  } else if (!x) {
    return fail(EBM_EINVAL, "%s: state pointer is NULL", who);
  }
  if (!v) return fail(EBM_EINVAL, "%s: velocity pointer is NULL", who);
  if (mlp && n_chains < 0) return fail(EBM_EINVAL, "%s: bad shape [%lld, %d]", who, (long long)n_chains, dim);
  if (k_steps < 1 || thin < 1) return fail(EBM_EINVAL, "%s: k_steps=%d thin=%d (both must be >= 1)", who, k_steps, thin);
  if (!(h > 0.0) || !(gamma > 0.0) || !(temperature > 0.0) || !std::isfinite(h) || !std::isfinite(gamma) || !std::isfinite(temperature))
    return fail(EBM_EINVAL, "%s: h=%g gamma=%g temperature=%g (all must be positive and finite)", who, h, gamma, temperature);
  if (int r = mlp ? wide_mlp_check_shape(who, energy->n_comp, dim) : kinetic_check_geometry(dim)) return r;
  if (mass) {
    if (int r = check_chain_mass(*mass, who)) return r;
  }
  if (n_chains == 0) return 0;
  if ((mlp && !aligned16(x)) || !aligned16(v) || (traj && !aligned16(traj)) || (noise && !aligned16(noise)))
    return fail(EBM_EINVAL, "%s: pointers must be 16-byte aligned", who);
  const KineticChainReq q = kinetic_request(energy, x, v, n_chains, dim, k_steps, h, gamma, temperature, draw_v0, thin, traj, noise,
                                            seed, offset);
  if (mass) {
    const KineticMassChainReq m{q, *mass};
    return mlp ? kinetic_mass_mlp_chain_launch(m, (hipStream_t)stream) : kinetic_mass_chain_launch(m, (hipStream_t)stream);
  }
  return mlp ? kinetic_mlp_chain_launch(q, (hipStream_t)stream) : kinetic_chain_launch(q, (hipStream_t)stream);
}

int ebm_kinetic_chain_f32(const ebm_energy_t* energy, float* x, float* v, int64_t n_chains, int32_t dim, int32_t k_steps,
                          double h, double gamma, double temperature, int32_t draw_v0, int32_t thin, float* traj,
                          const float* noise, uint64_t seed, uint64_t offset, void* stream) {
  return kinetic_chain_impl("ebm_kinetic_chain_f32", false, energy, x, v, n_chains, dim, k_steps, h, gamma, temperature, draw_v0, thin,
                            traj, noise, seed, offset, stream);
}

int ebm_kinetic_chain_mass_f32(const ebm_energy_t* energy, float* x, float* v, int64_t n_chains, int32_t dim, int32_t k_steps,
                               double h, double gamma, double temperature, int32_t mass_kind, double mass_scalar,
                               const float* mass_diag, int32_t draw_v0, int32_t thin, float* traj, const float* noise, uint64_t seed,
                               uint64_t offset, void* stream) {
  const ChainMass mass{mass_kind, mass_scalar, mass_diag};
  return kinetic_chain_impl("ebm_kinetic_chain_mass_f32", false, energy, x, v, n_chains, dim, k_steps, h, gamma, temperature, draw_v0,
                            thin, traj, noise, seed, offset, stream, &mass);
}

int ebm_kinetic_mlp_chain_f32(const ebm_energy_t* energy, float* x, float* v, int64_t n_chains, int32_t dim, int32_t k_steps,
                              double h, double gamma, double temperature, int32_t draw_v0, int32_t thin, float* traj,
                              const float* noise, uint64_t seed, uint64_t offset, void* stream) {
  return kinetic_chain_impl("ebm_kinetic_mlp_chain_f32", true, energy, x, v, n_chains, dim, k_steps, h, gamma, temperature, draw_v0,
                            thin, traj, noise, seed, offset, stream);
}

int ebm_kinetic_mlp_chain_mass_f32(const ebm_energy_t* energy, float* x, float* v, int64_t n_chains, int32_t dim, int32_t k_steps,
                                   double h, double gamma, double temperature, int32_t mass_kind, double mass_scalar,
                                   const float* mass_diag, int32_t draw_v0, int32_t thin, float* traj, const float* noise,
                                   uint64_t seed, uint64_t offset, void* stream) {
  const ChainMass mass{mass_kind, mass_scalar, mass_diag};
  return kinetic_chain_impl("ebm_kinetic_mlp_chain_mass_f32", true, energy, x, v, n_chains, dim, k_steps, h, gamma, temperature,
                            draw_v0, thin, traj, noise, seed, offset, stream, &mass);
}

// The request of both generalized-HMC entries: the constants of the refresh over one trajectory's time eps L, formed in double,
// each rounded once (gamma = +inf: c1 = 0 and c2 = sqrt_temp exactly)
static GhmcChainReq ghmc_request(const ebm_energy_t* energy, float* x, float* v, int64_t n_chains, int32_t dim, int32_t n_mh,
                                 int32_t n_leapfrog, double eps, double gamma, double temperature, int32_t draw_v0, int32_t thin,
                                 float* traj, uint8_t* accept_mask, const float* noise, const float* u, uint64_t seed,
                                 uint64_t offset) {
  const double span = gamma * eps * (double)n_leapfrog;
  const float sqrt_temp = (float)sqrt(temperature);
  const float c1 = std::isinf(gamma) ? 0.0f : (float)exp(-span);
  const float c2 = std::isinf(gamma) ? sqrt_temp : (float)sqrt(temperature * (-expm1(-2.0 * span)));
  const float beta = (float)(1.0 / temperature);
  return GhmcChainReq{*energy, x, v, n_chains, dim, n_mh, n_leapfrog, (float)eps, c1, c2, sqrt_temp, beta, draw_v0 != 0, thin, traj,
                      accept_mask, noise, u, seed, offset};
}

// What both generalized-HMC entries ask of the step counts and of the walk's parameters, adjacent in both
// (gamma = +inf is allowed: a full refresh, the HMC transition)
static int check_ghmc_parameters(int32_t n_mh, int32_t n_leapfrog, int32_t thin, double eps, double gamma, double temperature,
                                 const char* who) {
  if (n_mh < 1 || n_leapfrog < 1 || thin < 1)
    return fail(EBM_EINVAL, "%s: n_mh=%d n_leapfrog=%d thin=%d (all must be >= 1)", who, n_mh, n_leapfrog, thin);
  if (!(eps > 0.0) || !(gamma > 0.0) || !(temperature > 0.0) || !std::isfinite(eps) || !std::isfinite(temperature))
    return fail(EBM_EINVAL, "%s: eps=%g gamma=%g temperature=%g (all must be positive; eps and temperature finite)", who, eps, gamma,
                temperature);
  return 0;
}

// (two entries, not one impl: each forms its request in its own body, where tests/test_ghmc_mlp.py reads it)
int ebm_ghmc_chain_f32(const ebm_energy_t* energy, float* x, float* v, int64_t n_chains, int32_t dim, int32_t n_mh,
                       int32_t n_leapfrog, double eps, double gamma, double temperature, int32_t draw_v0, int32_t thin,
                       float* traj, uint8_t* accept_mask, const float* noise, const float* u, uint64_t seed, uint64_t offset,
                       void* stream) {
  const char* who = "ebm_ghmc_chain_f32";
  if (energy && energy->kind == EBM_ENERGY_MLP)
    return fail(EBM_EKIND, "%s: the MLP energy has no generalized-HMC kernel (the sampler's eager route takes it)", who);
  if (int r = check_energy(energy, dim, who)) return r;
  if (int r = ghmc_check_geometry(dim)) return r;  // (in front of check_state: dim < 1 is EBM_EDIM here, as dim > 256 is)
  if (int r = check_state(x, n_chains, dim, who)) return r;
  if (!v) return fail(EBM_EINVAL, "%s: velocity pointer is NULL", who);
  if (int r = check_ghmc_parameters(n_mh, n_leapfrog, thin, eps, gamma, temperature, who)) return r;
  if (n_chains == 0) return 0;
  if (!aligned16(v) || (traj && !aligned16(traj)) || (noise && !aligned16(noise)))
    return fail(EBM_EINVAL, "%s: pointers must be 16-byte aligned", who);
  return ghmc_chain_launch(ghmc_request(energy, x, v, n_chains, dim, n_mh, n_leapfrog, eps, gamma, temperature, draw_v0, thin, traj,
                                        accept_mask, noise, u, seed, offset),
                           (hipStream_t)stream);
}

// (the checks of ebm_ghmc_chain_f32 in its order, the mass behind the walk's parameters)
int ebm_ghmc_chain_mass_f32(const ebm_energy_t* energy, float* x, float* v, int64_t n_chains, int32_t dim, int32_t n_mh,
                            int32_t n_leapfrog, double eps, double gamma, double temperature, int32_t mass_kind, double mass_scalar,
                            const float* mass_diag, int32_t draw_v0, int32_t thin, float* traj, uint8_t* accept_mask,
                            const float* noise, const float* u, uint64_t seed, uint64_t offset, void* stream) {
  const char* who = "ebm_ghmc_chain_mass_f32";
  if (energy && energy->kind == EBM_ENERGY_MLP)
    return fail(EBM_EKIND, "%s: the MLP energy has no generalized-HMC kernel (the sampler's eager route takes it)", who);
  if (int r = check_energy(energy, dim, who)) return r;
  if (int r = ghmc_check_geometry(dim)) return r;
  if (int r = check_state(x, n_chains, dim, who)) return r;
  if (!v) return fail(EBM_EINVAL, "%s: velocity pointer is NULL", who);
  if (int r = check_ghmc_parameters(n_mh, n_leapfrog, thin, eps, gamma, temperature, who)) return r;
  const ChainMass mass{mass_kind, mass_scalar, mass_diag};
  if (int r = check_chain_mass(mass, who)) return r;
  if (n_chains == 0) return 0;
  if (!aligned16(v) || (traj && !aligned16(traj)) || (noise && !aligned16(noise)))
    return fail(EBM_EINVAL, "%s: pointers must be 16-byte aligned", who);
  return ghmc_mass_chain_launch(GhmcMassChainReq{ghmc_request(energy, x, v, n_chains, dim, n_mh, n_leapfrog, eps, gamma, temperature,
                                                              draw_v0, thin, traj, accept_mask, noise, u, seed, offset),
                                                 mass},
                                (hipStream_t)stream);
}

int ebm_ghmc_mlp_chain_f32(const ebm_energy_t* energy, float* x, float* v, int64_t n_chains, int32_t dim, int32_t n_mh,
                           int32_t n_leapfrog, double eps, double gamma, double temperature, int32_t draw_v0, int32_t thin,
                           float* traj, uint8_t* accept_mask, const float* noise, const float* u, uint64_t seed, uint64_t offset,
                           void* stream) {
  const char* who = "ebm_ghmc_mlp_chain_f32";
  if (int r = check_mlp_walk(energy, dim, who, "ebm_ghmc_chain_f32")) return r;
  // (the dim range is wide_mlp_check_shape's to refuse)
  if (!x) return fail(EBM_EINVAL, "%s: state pointer is NULL", who);
  if (!v) return fail(EBM_EINVAL, "%s: velocity pointer is NULL", who);
  if (n_chains < 0) return fail(EBM_EINVAL, "%s: bad shape [%lld, %d]", who, (long long)n_chains, dim);
  if (int r = check_ghmc_parameters(n_mh, n_leapfrog, thin, eps, gamma, temperature, who)) return r;
  if (int r = wide_mlp_check_shape(who, energy->n_comp, dim)) return r;
  if (n_chains == 0) return 0;
  if (!aligned16(x) || !aligned16(v) || (traj && !aligned16(traj)) || (noise && !aligned16(noise)))
    return fail(EBM_EINVAL, "%s: pointers must be 16-byte aligned", who);
  return ghmc_mlp_chain_launch(ghmc_request(energy, x, v, n_chains, dim, n_mh, n_leapfrog, eps, gamma, temperature, draw_v0, thin,
                                            traj, accept_mask, noise, u, seed, offset),
                               (hipStream_t)stream);
}

// (the checks of ebm_ghmc_mlp_chain_f32 in its order, the mass behind the shape rule and in front of the empty call)
int ebm_ghmc_mlp_chain_mass_f32(const ebm_energy_t* energy, float* x, float* v, int64_t n_chains, int32_t dim, int32_t n_mh,
                                int32_t n_leapfrog, double eps, double gamma, double temperature, int32_t mass_kind,
                                double mass_scalar, const float* mass_diag, int32_t draw_v0, int32_t thin, float* traj,
                                uint8_t* accept_mask, const float* noise, const float* u, uint64_t seed, uint64_t offset,
                                void* stream) {
  const char* who = "ebm_ghmc_mlp_chain_mass_f32";
  if (int r = check_mlp_walk(energy, dim, who, "ebm_ghmc_chain_mass_f32")) return r;
  // (the dim range is wide_mlp_check_shape's to refuse)
  if (!x) return fail(EBM_EINVAL, "%s: state pointer is NULL", who);
  if (!v) return fail(EBM_EINVAL, "%s: velocity pointer is NULL", who);
  if (n_chains < 0) return fail(EBM_EINVAL, "%s: bad shape [%lld, %d]", who, (long long)n_chains, dim);
  if (int r = check_ghmc_parameters(n_mh, n_leapfrog, thin, eps, gamma, temperature, who)) return r;
  if (int r = wide_mlp_check_shape(who, energy->n_comp, dim)) return r;
  const ChainMass mass{mass_kind, mass_scalar, mass_diag};
  if (int r = check_chain_mass(mass, who)) return r;
  if (n_chains == 0) return 0;
  if (!aligned16(x) || !aligned16(v) || (traj && !aligned16(traj)) || (noise && !aligned16(noise)))
    return fail(EBM_EINVAL, "%s: pointers must be 16-byte aligned", who);
  return ghmc_mass_mlp_chain_launch(GhmcMassChainReq{ghmc_request(energy, x, v, n_chains, dim, n_mh, n_leapfrog, eps, gamma,
                                                                  temperature, draw_v0, thin, traj, accept_mask, noise, u, seed,
                                                                  offset),
                                                     mass},
                                    (hipStream_t)stream);
}

// (the checks of ebm_ghmc_chain_f32 in its order, eps0 in the place of eps; the adaptation's own behind the walk's parameters)
int ebm_ghmc_adapt_chain_f32(const ebm_energy_t* energy, float* x, float* v, int64_t n_chains, int32_t dim, int32_t n_mh,
                             int32_t n_leapfrog, double eps0, double target_accept, double mu, double eps_min, double eps_max,
                             int32_t n_adapt, int32_t init_da, float* da, const float* da_table, float* eps_trace,
                             float* alpha_mean, double gamma, double temperature, int32_t draw_v0, int32_t thin, float* traj,
                             uint8_t* accept_mask, const float* noise, const float* u, uint64_t seed, uint64_t offset,
                             void* stream) {
  const char* who = "ebm_ghmc_adapt_chain_f32";
  if (energy && energy->kind == EBM_ENERGY_MLP)
    return fail(EBM_EKIND, "%s: the MLP energy has no generalized-HMC kernel (the sampler's eager route takes it)", who);
  if (int r = check_energy(energy, dim, who)) return r;
  if (int r = ghmc_check_geometry(dim)) return r;
  if (int r = check_state(x, n_chains, dim, who)) return r;
  if (!v) return fail(EBM_EINVAL, "%s: velocity pointer is NULL", who);
  if (int r = check_ghmc_parameters(n_mh, n_leapfrog, thin, eps0, gamma, temperature, who)) return r;
  const GhmcAdaptChainReq q{*energy, x, v, n_chains, dim, n_mh, n_leapfrog, eps0, gamma, temperature, target_accept, mu, eps_min,
                            eps_max, n_adapt, init_da, da, da_table, draw_v0 != 0, thin, traj, accept_mask, eps_trace, alpha_mean,
                            noise, u, seed, offset};
  if (int r = ghmc_adapt_check(q, who)) return r;
  if (n_chains == 0) return 0;
  if (!aligned16(v) || (traj && !aligned16(traj)) || (noise && !aligned16(noise)))
    return fail(EBM_EINVAL, "%s: pointers must be 16-byte aligned", who);
  return ghmc_adapt_chain_launch(q, (hipStream_t)stream);
}

// (the checks of ebm_ghmc_adapt_chain_f32 in its order, then the mass, all in front of the empty call)
int ebm_ghmc_adapt_chain_mass_f32(const ebm_energy_t* energy, float* x, float* v, int64_t n_chains, int32_t dim, int32_t n_mh,
                                  int32_t n_leapfrog, double eps0, double target_accept, double mu, double eps_min, double eps_max,
                                  int32_t n_adapt, int32_t init_da, float* da, const float* da_table, float* eps_trace,
                                  float* alpha_mean, double gamma, double temperature, int32_t mass_kind, double mass_scalar,
                                  const float* mass_diag, int32_t draw_v0, int32_t thin, float* traj, uint8_t* accept_mask,
                                  const float* noise, const float* u, uint64_t seed, uint64_t offset, void* stream) {
  const char* who = "ebm_ghmc_adapt_chain_mass_f32";
  if (energy && energy->kind == EBM_ENERGY_MLP)
    return fail(EBM_EKIND, "%s: the MLP energy has no generalized-HMC kernel (the sampler's eager route takes it)", who);
  if (int r = check_energy(energy, dim, who)) return r;
  if (int r = ghmc_check_geometry(dim)) return r;
  if (int r = check_state(x, n_chains, dim, who)) return r;
  if (!v) return fail(EBM_EINVAL, "%s: velocity pointer is NULL", who);
  if (int r = check_ghmc_parameters(n_mh, n_leapfrog, thin, eps0, gamma, temperature, who)) return r;
  const GhmcAdaptChainReq q{*energy, x, v, n_chains, dim, n_mh, n_leapfrog, eps0, gamma, temperature, target_accept, mu, eps_min,
                            eps_max, n_adapt, init_da, da, da_table, draw_v0 != 0, thin, traj, accept_mask, eps_trace, alpha_mean,
                            noise, u, seed, offset};
  if (int r = ghmc_adapt_check(q, who)) return r;
  const ChainMass mass{mass_kind, mass_scalar, mass_diag};
  if (int r = check_chain_mass(mass, who)) return r;
  if (n_chains == 0) return 0;
  if (!aligned16(v) || (traj && !aligned16(traj)) || (noise && !aligned16(noise)))
    return fail(EBM_EINVAL, "%s: pointers must be 16-byte aligned", who);
  return ghmc_adapt_mass_chain_launch(GhmcAdaptMassChainReq{q, mass}, (hipStream_t)stream);
}

// Both running-moments entries of the two walkers, as the underdamped pair; the analytic entry's geometry stands in front of its
// state (dim < 1 is EBM_EDIM there, as dim > 256 is)
static int kinetic_moments_impl(const char* who, bool mlp, const ebm_energy_t* energy, float* x, float* v, int64_t n_chains,
                                int32_t dim, int32_t sampler, int32_t k_steps, int32_t burn_in, int32_t n_leapfrog, double step,
                                double gamma, double temperature, int32_t draw_v0, const float* recip, float* mom, float* e_mom,
                                float* v2_mom, float* traj, float* e_traj, float* v_traj, uint8_t* accept_mask,
                                uint32_t* accept_count, const float* noise, const float* u, uint64_t seed, uint64_t offset,
                                void* stream) {
  if (!mlp && energy && energy->kind == EBM_ENERGY_MLP)
    return fail(EBM_EKIND, "%s: the MLP energy has no running-moments kernel (the samplers' eager route takes it)", who);
  if (int r = mlp ? check_mlp_walk(energy, dim, who, "ebm_kinetic_moments_f32") : check_energy(energy, dim, who)) return r;
  if (!mlp) {
    if (int r = kinetic_moments_check_geometry(dim)) return r;
    if (int r = check_state(x, n_chains, dim, who)) return r;
  } else if (!x) {
    return fail(EBM_EINVAL, "%s: state pointer is NULL", who);
  }
  if (!v) return fail(EBM_EINVAL, "%s: velocity pointer is NULL", who);
  if (mlp && n_chains < 0) return fail(EBM_EINVAL, "%s: bad shape [%lld, %d]", who, (long long)n_chains, dim);
  if (sampler != 0 && sampler != 1) return fail(EBM_EINVAL, "%s: sampler=%d (0 = BAOAB, 1 = GHMC)", who, sampler);
  const bool ghmc = sampler == 1;
  if (int r = check_moments_window(k_steps, burn_in, who)) return r;
  // (GHMC: gamma = +inf is allowed, a full refresh)
  if (!(step > 0.0) || !(gamma > 0.0) || !(temperature > 0.0) || !std::isfinite(step) || !std::isfinite(temperature) ||
      (!ghmc && !std::isfinite(gamma)))
    return fail(EBM_EINVAL, "%s: step=%g gamma=%g temperature=%g (all must be positive; finite, but for GHMC's gamma)", who, step,
                gamma, temperature);
  if (ghmc && n_leapfrog < 1) return fail(EBM_EINVAL, "%s: n_leapfrog=%d", who, n_leapfrog);
  if (ghmc && (v2_mom || v_traj)) return fail(EBM_EINVAL, "%s: v2_mom / v_traj are BAOAB outputs (sampler = 0)", who);
  if (!recip || !mom) return fail(EBM_EINVAL, "%s: recip / mom is NULL", who);
  if (mlp)
    if (int r = wide_mlp_check_shape(who, energy->n_comp, dim)) return r;
  if (n_chains == 0) return 0;
  if ((mlp && !aligned16(x)) || !aligned16(v) || !aligned16(mom) || (v2_mom && !aligned16(v2_mom)) || (traj && !aligned16(traj)) ||
      (v_traj && !aligned16(v_traj)) || (noise && !aligned16(noise)))
    return fail(EBM_EINVAL, "%s: pointers must be 16-byte aligned", who);
  // the walkers' constants by the host code of the two plain entries
  const auto launch = mlp ? kinetic_moments_mlp_chain_launch : kinetic_moments_chain_launch;
  if (ghmc) {
    const GhmcChainReq g = ghmc_request(energy, x, v, n_chains, dim, k_steps, n_leapfrog, step, gamma, temperature, draw_v0, 1,
                                        nullptr, accept_mask, noise, u, seed, offset);
    const KineticMomentsChainReq q{*energy, x, v, n_chains, dim, true, k_steps, burn_in, n_leapfrog, 0.0f, g.eps, g.c1, g.c2,
                                   g.sqrt_temp, g.beta, draw_v0 != 0, recip, mom, e_mom, nullptr, traj, e_traj, nullptr,
                                   accept_mask, accept_count, noise, u, seed, offset};
    return launch(q, (hipStream_t)stream);
  }
  const KineticChainReq b = kinetic_request(energy, x, v, n_chains, dim, k_steps, step, gamma, temperature, draw_v0, 1, nullptr,
                                            noise, seed, offset);
  const KineticMomentsChainReq q{*energy, x, v, n_chains, dim, false, k_steps, burn_in, n_leapfrog, b.hh, 0.0f, b.c1, b.c2,
                                 b.sqrt_temp, 0.0f, draw_v0 != 0, recip, mom, e_mom, v2_mom, traj, e_traj, v_traj, nullptr, nullptr,
                                 noise, nullptr, seed, offset};
  return launch(q, (hipStream_t)stream);
}

int ebm_kinetic_moments_f32(const ebm_energy_t* energy, float* x, float* v, int64_t n_chains, int32_t dim, int32_t sampler,
                            int32_t k_steps, int32_t burn_in, int32_t n_leapfrog, double step, double gamma, double temperature,
                            int32_t draw_v0, const float* recip, float* mom, float* e_mom, float* v2_mom, float* traj,
                            float* e_traj, float* v_traj, uint8_t* accept_mask, uint32_t* accept_count, const float* noise,
                            const float* u, uint64_t seed, uint64_t offset, void* stream) {
  return kinetic_moments_impl("ebm_kinetic_moments_f32", false, energy, x, v, n_chains, dim, sampler, k_steps, burn_in, n_leapfrog,
                              step, gamma, temperature, draw_v0, recip, mom, e_mom, v2_mom, traj, e_traj, v_traj, accept_mask,
                              accept_count, noise, u, seed, offset, stream);
}

int ebm_kinetic_moments_mlp_f32(const ebm_energy_t* energy, float* x, float* v, int64_t n_chains, int32_t dim, int32_t sampler,
                                int32_t k_steps, int32_t burn_in, int32_t n_leapfrog, double step, double gamma,
                                double temperature, int32_t draw_v0, const float* recip, float* mom, float* e_mom, float* v2_mom,
                                float* traj, float* e_traj, float* v_traj, uint8_t* accept_mask, uint32_t* accept_count,
                                const float* noise, const float* u, uint64_t seed, uint64_t offset, void* stream) {
  return kinetic_moments_impl("ebm_kinetic_moments_mlp_f32", true, energy, x, v, n_chains, dim, sampler, k_steps, burn_in,
                              n_leapfrog, step, gamma, temperature, draw_v0, recip, mom, e_mom, v2_mom, traj, e_traj, v_traj,
                              accept_mask, accept_count, noise, u, seed, offset, stream);
}

int ebm_leapfrog_kick_drift_f32(const float* x, const float* p, const float* force, float* x_new,
                                float* p_half, int64_t n_chains, int32_t dim, float eps,
                                int32_t mass_kind, double mass_scalar, const float* mass_diag,
                                int32_t safe, void* stream) {
  const char* who = "ebm_leapfrog_kick_drift_f32";
  if (n_chains < 0 || dim < 1) return fail(EBM_EINVAL, "%s: bad shape", who);
  if (n_chains == 0) return 0;
  if (!x || !p || !force || !x_new || !p_half) return fail(EBM_EINVAL, "%s: NULL pointer", who);
  if (mass_kind == EBM_MASS_DIAG && !mass_diag) return fail(EBM_EINVAL, "%s: diagonal mass is NULL", who);
  if (!aligned16(x) || !aligned16(p) || !aligned16(force) || !aligned16(x_new) || !aligned16(p_half))
    return fail(EBM_EINVAL, "%s: pointers must be 16-byte aligned", who);
  return launch_leapfrog_kick_drift(x, p, force, x_new, p_half, n_chains, dim, eps, mass_kind,
                                    mass_scalar, mass_diag, safe, (hipStream_t)stream);
}

int ebm_leapfrog_kick_f32(float* x_new, const float* p_half, const float* force, float* p_new,
                          int64_t n_elem, float eps, int32_t safe, void* stream) {
  const char* who = "ebm_leapfrog_kick_f32";
  if (n_elem < 0) return fail(EBM_EINVAL, "%s: n_elem < 0", who);
  if (n_elem == 0) return 0;
  if (!x_new || !p_half || !force || !p_new) return fail(EBM_EINVAL, "%s: NULL pointer", who);
  if (!aligned16(x_new) || !aligned16(p_half) || !aligned16(force) || !aligned16(p_new))
    return fail(EBM_EINVAL, "%s: pointers must be 16-byte aligned", who);
  return launch_leapfrog_kick(x_new, p_half, force, p_new, n_elem, eps, safe, (hipStream_t)stream);
}

int ebm_hmc_accept_f32(float* x, const float* x_prop, const float* h0, const float* h1,
                       const float* u, uint8_t* accept_mask, uint32_t* accept_count,
                       int64_t n_chains, int32_t dim, uint64_t seed, uint64_t offset, void* stream) {
  const char* who = "ebm_hmc_accept_f32";
  if (n_chains < 0 || dim < 1) return fail(EBM_EINVAL, "%s: bad shape", who);
  if (n_chains == 0) return 0;
  if (!x || !x_prop || !h0 || !h1) return fail(EBM_EINVAL, "%s: NULL pointer", who);
  return launch_hmc_accept(x, x_prop, h0, h1, u, accept_mask, accept_count, n_chains, dim, seed,
                           offset, nullptr, (hipStream_t)stream);
}

int ebm_hmc_accept_dev_f32(float* x, const float* x_prop, const float* h0, const float* h1,
                           uint8_t* accept_mask, uint32_t* accept_count, int64_t n_chains, int32_t dim,
                           const uint64_t* rng_state, uint64_t step_delta, void* stream) {
  const char* who = "ebm_hmc_accept_dev_f32";
  if (n_chains < 0 || dim < 1) return fail(EBM_EINVAL, "%s: bad shape", who);
  if (n_chains == 0) return 0;
  if (!x || !x_prop || !h0 || !h1 || !rng_state) return fail(EBM_EINVAL, "%s: NULL pointer", who);
  return launch_hmc_accept(x, x_prop, h0, h1, nullptr, accept_mask, accept_count, n_chains, dim, 0,
                           step_delta, rng_state, (hipStream_t)stream);
}

int ebm_descent_chain_f32(const ebm_energy_t* energy, float* x, int64_t n_chains, int32_t dim,
                          int32_t k_steps, float eta, const float* eta_table, int32_t nesterov,
                          float momentum, int32_t thin, float* traj, void* stream) {
  const char* who = "ebm_descent_chain_f32";
  if (int r = check_energy(energy, dim, who)) return r;
  if (int r = reject_mlp(energy, who)) return r;
  if (int r = check_state(x, n_chains, dim, who)) return r;
  if (k_steps < 0 || thin < 1) return fail(EBM_EINVAL, "%s: k_steps=%d thin=%d", who, k_steps, thin);
  if (n_chains == 0 || k_steps == 0) return 0;
  if (traj && !aligned16(traj)) return fail(EBM_EINVAL, "%s: traj must be 16-byte aligned", who);
  return launch_descent_chain(*energy, x, n_chains, dim, k_steps, eta, eta_table, nesterov, momentum, thin,
                              traj, (hipStream_t)stream);
}

int ebm_descent_step_f32(const float* x, const float* grad, float* v, float* out, int64_t n_elem,
                         float eta, float momentum, void* stream) {
  const char* who = "ebm_descent_step_f32";
  if (n_elem < 0) return fail(EBM_EINVAL, "%s: n_elem < 0", who);
  if (n_elem == 0) return 0;
  if (!x || !grad || !out) return fail(EBM_EINVAL, "%s: NULL pointer", who);
  if (!aligned16(x) || !aligned16(grad) || !aligned16(out) || (v && !aligned16(v)))
    return fail(EBM_EINVAL, "%s: pointers must be 16-byte aligned", who);
  return launch_descent_step(x, grad, v, out, n_elem, eta, momentum, (hipStream_t)stream);
}

int ebm_lookahead_f32(const float* x, const float* v, float* out, int64_t n_elem, float momentum,
                      void* stream) {
  const char* who = "ebm_lookahead_f32";
  if (n_elem < 0) return fail(EBM_EINVAL, "%s: n_elem < 0", who);
  if (n_elem == 0) return 0;
  if (!x || !v || !out) return fail(EBM_EINVAL, "%s: NULL pointer", who);
  if (!aligned16(x) || !aligned16(v) || !aligned16(out)) return fail(EBM_EINVAL, "%s: pointers must be 16-byte aligned", who);
  return launch_lookahead(x, v, out, n_elem, momentum, (hipStream_t)stream);
}

int ebm_pcd_gather_f32(const float* buffer, int64_t buffer_size, int32_t dim, float* out, int64_t batch,
                       int64_t stride, const int64_t* offsets, int64_t* rows_out, uint64_t seed,
                       uint64_t offset, void* stream) {
  const char* who = "ebm_pcd_gather_f32";
  if (buffer_size < 1 || dim < 1 || batch < 0 || stride < 1 || stride > 0x7fffffffLL)
    return fail(EBM_EINVAL, "%s: bad sizes (buffer %lld, dim %d, batch %lld, stride %lld)", who, (long long)buffer_size, dim,
                (long long)batch, (long long)stride);
  if (batch == 0) return 0;
  if (!buffer || !out) return fail(EBM_EINVAL, "%s: NULL pointer", who);
  return launch_pcd_gather(buffer, buffer_size, dim, out, batch, stride, offsets, rows_out, seed, offset, nullptr,
                           (hipStream_t)stream);
}

int ebm_pcd_gather_dev_f32(const float* buffer, int64_t buffer_size, int32_t dim, float* out, int64_t batch,
                           int64_t stride, int64_t* rows_out, const uint64_t* rng_state, uint64_t step_delta,
                           void* stream) {
  const char* who = "ebm_pcd_gather_dev_f32";
  if (buffer_size < 1 || dim < 1 || batch < 0 || stride < 1 || stride > 0x7fffffffLL)
    return fail(EBM_EINVAL, "%s: bad sizes (buffer %lld, dim %d, batch %lld, stride %lld)", who, (long long)buffer_size, dim,
                (long long)batch, (long long)stride);
  if (batch == 0) return 0;
  if (!buffer || !out || !rng_state) return fail(EBM_EINVAL, "%s: NULL pointer", who);
  return launch_pcd_gather(buffer, buffer_size, dim, out, batch, stride, nullptr, rows_out, 0, step_delta, rng_state,
                           (hipStream_t)stream);
}

int64_t ebm_cd_loss_work_bytes(void) { return cd_loss_work_bytes(); }

int ebm_cd_loss_f32(const float* e_both, int64_t n, float reg, void* work, float* loss_out, float* finite_out, void* stream) {
  const char* who = "ebm_cd_loss_f32";
  if (n < 1) return fail(EBM_EINVAL, "%s: n < 1", who);
  if (!e_both || !work || !loss_out || !finite_out || (reinterpret_cast<uintptr_t>(work) & 7) != 0)
    return fail(EBM_EINVAL, "%s: NULL pointer, or work not 8-byte aligned", who);
  return launch_cd_loss(e_both, n, reg, work, loss_out, finite_out, (hipStream_t)stream);
}

int ebm_cd_loss_backward_f32(const float* e_both, int64_t n, float reg, const float* upstream, const float* finite, float* seed_out,
                             void* stream) {
  const char* who = "ebm_cd_loss_backward_f32";
  if (n < 1) return fail(EBM_EINVAL, "%s: n < 1", who);
  if (!e_both || !upstream || !finite || !seed_out) return fail(EBM_EINVAL, "%s: NULL pointer", who);
  return launch_cd_loss_seed(e_both, n, reg, upstream, finite, seed_out, (hipStream_t)stream);
}

int ebm_pcd_start_points_f32(const float* buffer, int64_t buffer_size, int32_t dim, float* out, int64_t batch, int64_t stride,
                             int64_t n_noise, float noise_scale, uint64_t seed, uint64_t step, const uint64_t* rng_state, void* stream) {
  const char* who = "ebm_pcd_start_points_f32";
  if (buffer_size < 1 || dim < 1 || batch < 0 || batch > 0x7fffffffLL || stride < 1 || stride > 0x7fffffffLL || n_noise < 0 || n_noise > batch)
    return fail(EBM_EINVAL, "%s: bad sizes (buffer %lld, dim %d, batch %lld, stride %lld, n_noise %lld)", who, (long long)buffer_size, dim,
                (long long)batch, (long long)stride, (long long)n_noise);
  if (batch == 0) return 0;
  if (!buffer || !out) return fail(EBM_EINVAL, "%s: NULL pointer", who);
  return launch_pcd_start_points(buffer, buffer_size, dim, out, batch, stride, n_noise, noise_scale, seed, step, rng_state, (hipStream_t)stream);
}

int ebm_gmm_active_columns_i32(const float* means, int32_t n_comp, int32_t dim, int32_t* out, void* stream) {
  const char* who = "ebm_gmm_active_columns_i32";
  if (n_comp < 1 || dim < 4 || dim > 32 || (dim % 4) != 0)
    return fail(EBM_EINVAL, "%s: bad sizes (n_comp %d, dim %d: a multiple of 4 up to 32)", who, n_comp, dim);
  if (!means || !out) return fail(EBM_EINVAL, "%s: NULL pointer", who);
  return launch_gmm_active_columns(means, n_comp, dim, out, (hipStream_t)stream);
}

int ebm_pcd_scatter_f32(float* buffer, int64_t buffer_size, int32_t dim, const float* samples, int64_t batch,
                        int64_t write_pos, void* stream) {
  const char* who = "ebm_pcd_scatter_f32";
  if (buffer_size < 1 || dim < 1 || batch < 0 || batch > buffer_size || write_pos < 0 || write_pos >= buffer_size)
    return fail(EBM_EINVAL, "%s: bad sizes (buffer %lld, batch %lld, write_pos %lld)", who, (long long)buffer_size,
                (long long)batch, (long long)write_pos);
  if (batch == 0) return 0;
  if (!buffer || !samples) return fail(EBM_EINVAL, "%s: NULL pointer", who);
  return launch_pcd_scatter(buffer, buffer_size, dim, samples, batch, write_pos, nullptr, (hipStream_t)stream);
}

int ebm_pcd_scatter_dev_f32(float* buffer, int64_t buffer_size, int32_t dim, const float* samples, int64_t batch,
                            const int64_t* write_pos, void* stream) {
  const char* who = "ebm_pcd_scatter_dev_f32";
  if (buffer_size < 1 || dim < 1 || batch < 0 || batch > buffer_size)
    return fail(EBM_EINVAL, "%s: bad sizes (buffer %lld, batch %lld)", who, (long long)buffer_size, (long long)batch);
  if (batch == 0) return 0;
  if (!buffer || !samples || !write_pos) return fail(EBM_EINVAL, "%s: NULL pointer", who);
  return launch_pcd_scatter(buffer, buffer_size, dim, samples, batch, 0, write_pos, (hipStream_t)stream);
}

int ebm_energy_grad_f32(const ebm_energy_t* energy, const float* x, int64_t n_chains, int32_t dim,
                        float* energy_out, float* grad_out, void* stream) {
  const char* who = "ebm_energy_grad_f32";
  if (int r = check_energy(energy, dim, who)) return r;
  if (int r = check_state(x, n_chains, dim, who)) return r;
  if (n_chains == 0) return 0;
  if (grad_out && !aligned16(grad_out)) return fail(EBM_EINVAL, "%s: grad_out must be 16-byte aligned", who);
  if (energy->kind == EBM_ENERGY_MLP)
    return launch_energy_grad_mlp(*energy, x, n_chains, dim, energy_out, grad_out, (hipStream_t)stream);
  if (energy->kind == EBM_ENERGY_GAUSSIAN && gauss_big_supported(dim)) {  // above 128 dims: one contraction pass on the matrix cores
    static const bool force_rows = ab_switch("EBM_GAUSS_ROWS");
    if (!force_rows) return launch_energy_grad_gauss_big(*energy, x, n_chains, dim, energy_out, grad_out, (hipStream_t)stream);
  }
  return launch_energy_grad(*energy, x, n_chains, dim, energy_out, grad_out, (hipStream_t)stream);
}

int ebm_mlp_backward_acts_f32(const ebm_energy_t* energy, const float* x, int64_t n_chains, int32_t dim, const float* seed,
                              float* energy_out, float* grad_out, float* acts, void* stream) {
  const char* who = "ebm_mlp_backward_acts_f32";
  if (int r = check_energy(energy, dim, who)) return r;
  if (int r = check_state(x, n_chains, dim, who)) return r;
  if (energy->kind != EBM_ENERGY_MLP) return fail(EBM_EKIND, "%s: EBM_ENERGY_MLP only", who);
  if (!energy->dev0) return fail(EBM_EINVAL, "%s: packed MLP parameters pointer is NULL", who);
  if ((energy->n_comp != 64 && energy->n_comp != 128) || dim < 1 || dim > 64)
    return fail(EBM_EDIM, "%s: hidden width 64 or 128 and dim <= 64 (got %d, %d)", who, energy->n_comp, dim);
  if (n_chains == 0) return 0;
  if (!acts || !aligned16(acts) || (grad_out && !aligned16(grad_out))) return fail(EBM_EINVAL, "%s: acts / grad_out must be 16-byte aligned pointers", who);
  if (((n_chains + 127) / 128 * 128) * 20 >= (1LL << 32)) return fail(EBM_EINVAL, "%s: too many rows for 32-bit lane offsets", who);  // (a bound kept from the [4][H][n] layout)
  return launch_mlp_backward_acts(energy->n_comp, energy->dev0, x, n_chains, dim, seed, energy_out, grad_out, acts, (hipStream_t)stream, who);
}

int64_t ebm_mlp_param_grads_work_f32(int32_t hidden, int32_t dim, int64_t n_rows) {
  if ((hidden != 64 && hidden != 128) || dim < 1 || dim > 64 || n_rows < 0) return 0;
  return mlp_param_grads_work_floats(hidden, dim, n_rows);
}

int ebm_mlp_param_grads_f32(const float* acts, int64_t n_rows, int32_t hidden, const float* x, int32_t dim, const float* seed,
                            const float* w3, float* work, int64_t work_floats, float* grads_out, void* stream) {
  const char* who = "ebm_mlp_param_grads_f32";
  if ((hidden != 64 && hidden != 128) || dim < 1 || dim > 64)
    return fail(EBM_EDIM, "%s: hidden width 64 or 128 and dim <= 64 (got %d, %d)", who, hidden, dim);
  if (n_rows < 1) return fail(EBM_EINVAL, "%s: no rows", who);
  if (!acts || !aligned16(acts) || !x || !grads_out || !work || !w3) return fail(EBM_EINVAL, "%s: NULL pointer, or acts not 16-byte aligned", who);
  if (work_floats < mlp_param_grads_work_floats(hidden, dim, n_rows))
    return fail(EBM_EINVAL, "%s: workspace of %lld floats, need ebm_mlp_param_grads_work_f32() = %lld", who, (long long)work_floats,
                (long long)mlp_param_grads_work_floats(hidden, dim, n_rows));
  return launch_mlp_param_grads(hidden, acts, x, n_rows, dim, seed, w3, work, grads_out, (hipStream_t)stream, who);
}

int ebm_chain_stats_f32(const float* x, int64_t n_chains, int32_t dim, float* mean_out,
                        float* var_out, double* work, void* stream) {
  const char* who = "ebm_chain_stats_f32";
  if (int r = check_state(x, n_chains, dim, who)) return r;
  if (!mean_out || !var_out || !work) return fail(EBM_EINVAL, "%s: NULL output/workspace", who);
  if (n_chains == 0) return fail(EBM_EINVAL, "%s: no chains", who);
  return launch_chain_stats(x, n_chains, dim, mean_out, var_out, work, (hipStream_t)stream);
}

int ebm_noise_fill_f32(float* out, int64_t n_elem, int32_t kind, uint64_t seed, uint64_t offset,
                       void* stream) {
  const char* who = "ebm_noise_fill_f32";
  if (n_elem < 0) return fail(EBM_EINVAL, "%s: n_elem < 0", who);
  if (n_elem == 0) return 0;
  if (!out || !aligned16(out)) return fail(EBM_EINVAL, "%s: out must be a 16-byte aligned pointer", who);
  if (kind < EBM_NOISE_NORMAL || kind > EBM_NOISE_RAW_U32) return fail(EBM_EINVAL, "%s: bad kind %d", who, kind);
  return launch_noise_fill(out, n_elem, kind, seed, offset, nullptr, (hipStream_t)stream);
}

int ebm_noise_fill_dev_f32(float* out, int64_t n_elem, int32_t kind, const uint64_t* rng_state,
                           uint64_t step_delta, void* stream) {
  const char* who = "ebm_noise_fill_dev_f32";
  if (n_elem < 0) return fail(EBM_EINVAL, "%s: n_elem < 0", who);
  if (n_elem == 0) return 0;
  if (!out || !aligned16(out)) return fail(EBM_EINVAL, "%s: out must be a 16-byte aligned pointer", who);
  if (!rng_state) return fail(EBM_EINVAL, "%s: rng_state is NULL", who);
  if (kind < EBM_NOISE_NORMAL || kind > EBM_NOISE_RAW_U32) return fail(EBM_EINVAL, "%s: bad kind %d", who, kind);
  return launch_noise_fill(out, n_elem, kind, 0, step_delta, rng_state, (hipStream_t)stream);
}

int ebm_diag_layout(const ebm_energy_t* energy, int32_t sampler, int64_t n_chains, int32_t dim, int32_t injected_noise,
                    int32_t with_traj, int64_t* n_blocks, int32_t* slots, int32_t* block_elems) {
  const char* who = "ebm_diag_layout";
  if (int r = check_energy(energy, dim, who)) return r;
  if (sampler < EBM_DIAG_LANGEVIN || sampler > EBM_DIAG_HMC) return fail(EBM_EINVAL, "%s: unknown sampler kind %d", who, sampler);
  if (n_chains < 1 || dim < 1 || !n_blocks || !slots || !block_elems)
    return fail(EBM_EINVAL, "%s: bad shape [%lld, %d] or NULL output", who, (long long)n_chains, dim);
  diag::DiagArgs d;
  if (plan_diag(*energy, sampler, n_chains, dim, injected_noise != 0, with_traj != 0, d) == kDiagNone)
    return fail(energy->kind == EBM_ENERGY_MLP ? EBM_EKIND : EBM_EDIM, "%s: no in-kernel diagnostics for this energy / dim %d", who,
                dim);
  *n_blocks = d.n_blocks;
  *slots = d.S;
  *block_elems = d.E;
  return 0;
}

int ebm_diag_finish_f32(const float* diag_partials, int32_t n_kept, int64_t n_blocks, int32_t slots, int32_t block_elems,
                        int64_t n_chains, int32_t dim, float* mean_out, float* var_out, float* energy_out, float* accept_out,
                        double* work, void* stream) {
  const char* who = "ebm_diag_finish_f32";
  if (n_kept < 0) return fail(EBM_EINVAL, "%s: n_kept < 0", who);
  if (n_kept == 0) return 0;
  if (!diag_partials || !mean_out || !var_out || !work) return fail(EBM_EINVAL, "%s: NULL records / outputs / workspace", who);
  if (block_elems < 0) {  // records of interleaved classes (shifted rows): -32 dim, 4 / gcd(dim, 4) classes
    const int K = diag::diag_classes(dim);
    if (n_chains < 1 || dim < 1 || K < 2 || block_elems != -32 * dim || slots != dim || n_blocks != ceil_div64(n_chains, 32 * (int64_t)K) * K)
      return fail(EBM_EINVAL, "%s: inconsistent interleaved layout (n_blocks %lld, slots %d, block_elems %d for [%lld, %d])", who,
                  (long long)n_blocks, slots, block_elems, (long long)n_chains, dim);
    return launch_diag_finish(diag_partials, n_kept, n_blocks, slots, block_elems, n_chains, dim, mean_out, var_out, energy_out,
                              accept_out, work, (hipStream_t)stream);
  }
  if (n_chains < 1 || dim < 1 || n_blocks < 1 || slots < 1 || block_elems < 1 || slots != (dim < block_elems ? dim : block_elems) ||
      (block_elems % dim != 0 && dim % block_elems != 0) || n_blocks != ceil_div64(n_chains * (int64_t)dim, block_elems))
    return fail(EBM_EINVAL, "%s: inconsistent layout (n_blocks %lld, slots %d, block_elems %d for [%lld, %d])", who,
                (long long)n_blocks, slots, block_elems, (long long)n_chains, dim);
  return launch_diag_finish(diag_partials, n_kept, n_blocks, slots, block_elems, n_chains, dim, mean_out, var_out, energy_out,
                            accept_out, work, (hipStream_t)stream);
}

int ebm_probe_valu_f32(float* out, int32_t blocks, int32_t iters, void* stream) {
  const char* who = "ebm_probe_valu_f32";
  if (!out || blocks < 1 || iters < 1) return fail(EBM_EINVAL, "%s: out is NULL or blocks/iters < 1", who);
  return launch_probe_valu(out, blocks, iters, (hipStream_t)stream);
}

int ebm_probe_issue_f32(float* out, int32_t blocks, int32_t iters, int32_t kind, void* stream) {
  const char* who = "ebm_probe_issue_f32";
  if (!out || blocks < 1 || iters < 1) return fail(EBM_EINVAL, "%s: out is NULL or blocks/iters < 1", who);
  if (kind < 0 || kind > 7) return fail(EBM_EINVAL, "%s: kind %d (0 fma | 1 mad_u64_u32 | 2 transcendental | 3 pk_fma | 4 bitop3 | 5 pk_fma, VGPR operands | 6 pk_mul | 7 the lean loop's mix)", who, kind);
  return launch_probe_issue(out, blocks, iters, kind, (hipStream_t)stream);
}

size_t ebm_mlp_w1_image_bytes(int32_t hidden, int32_t dim) { return mlp_w1_image_bytes(hidden, dim); }

size_t ebm_gauss_prec_image_bytes(int32_t dim) { return gauss_prec_image_bytes(dim); }

int ebm_gauss_prec_image_f32(const float* prec, int32_t dim, void* image, void* stream) {
  return launch_gauss_prec_image(prec, dim, image, (hipStream_t)stream, "ebm_gauss_prec_image_f32");
}

int ebm_mlp_w1_image_f32(const float* params, int32_t hidden, int32_t dim, void* image, void* stream) {
  return launch_mlp_w1_image(params, hidden, dim, image, (hipStream_t)stream, "ebm_mlp_w1_image_f32");
}

}  // extern "C"
