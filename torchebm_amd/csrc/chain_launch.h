// Host-side requests of the fused Langevin and HMC chain calls, and the one declaration of every chain launcher.
// The C-ABI entries (api.hip) validate a call and decode it into a request once; a launcher fills its kernel's own
// argument struct from the request.  A request never reaches a kernel.
#pragma once
#include <cmath>

#include "diag.h"
#include "ebm_common.h"

namespace ebm {

struct LangevinChainReq {
  const ebm_energy_t& e;
  float* x;
  int64_t n_chains;
  int32_t dim, k_steps;
  float eta, sqrt_eta, noise_coef;
  const float* coef_table;
  bool clamp, contracted;  // the flag word `clamp_on`, decoded: EBM_CHAIN_CLAMP, EBM_CHAIN_CONTRACTED
  float cmin, cmax;
  int32_t thin;
  float* traj;
  const float* noise;
  uint64_t seed, offset;
  float* diag_partials;     // null when no step is kept
  int heun;
  const uint64_t* rng_dev;  // ebm_langevin_chain_dev_f32: {seed, step} in device memory (MLP kernels only), else null
  // The start state [n_chains, dim], read-only; always set, == x for an in-place call.  ebm_langevin_chain_from_f32 passes another
  // buffer: the element-wise launchers load from it and store to x; for every other family the entry has copied it into x
  // before the request is routed, and the launcher sees src == x.
  const float* src;

  RngKey key() const { return RngKey{(uint32_t)seed, (uint32_t)(seed >> 32)}; }
  int32_t n_kept() const { return k_steps / thin; }
};

struct HmcChainReq {
  const ebm_energy_t& e;
  float* x;
  int64_t n_chains;
  int32_t dim, n_mh, n_leapfrog;
  float eps;
  const float* eps_table;
  int32_t mass_kind;
  double mass_scalar;
  const float* mass_diag;
  int32_t thin;
  float* traj;
  uint8_t* accept_mask;
  uint32_t* accept_count;
  const float* p_noise;
  const float* u;
  uint64_t seed, offset;
  float* diag_partials;  // null when no transition is kept

  RngKey key() const { return RngKey{(uint32_t)seed, (uint32_t)(seed >> 32)}; }
  int32_t n_kept() const { return n_mh / thin; }
};

struct TemperingChainReq {
  const ebm_energy_t& e;
  float* x;                 // the slot matrix [n_ladders * n_replicas, dim]
  int64_t n_ladders;
  int32_t n_replicas, dim, k_steps;
  float eta, sqrt_eta;
  const float* noise_coef;  // device [n_replicas]
  const float* beta;        // device [n_replicas]
  int32_t swap_every, thin;
  float* traj;
  uint32_t* swap_counts;
  const float* noise;
  const float* u;
  uint64_t seed, offset;

  RngKey key() const { return RngKey{(uint32_t)seed, (uint32_t)(seed >> 32)}; }
  int32_t n_kept() const { return k_steps / thin; }
};

struct TemperingHmcChainReq {
  const ebm_energy_t& e;
  float* x;                // the slot matrix [n_ladders * n_replicas, dim]
  int64_t n_ladders;
  int32_t n_replicas, dim, n_mh, n_leapfrog;
  const float* eps;        // device [n_replicas]: the slots' step sizes
  const float* sqrt_temp;  // device [n_replicas]
  const float* beta;       // device [n_replicas]
  int32_t swap_every, thin;
  float* traj;
  uint8_t* accept_mask;
  uint32_t* accept_counts;
  uint32_t* swap_counts;
  const float* p_noise;
  const float* u_accept;
  const float* u_swap;
  uint64_t seed, offset;

  RngKey key() const { return RngKey{(uint32_t)seed, (uint32_t)(seed >> 32)}; }
  int32_t n_kept() const { return n_mh / thin; }
};

struct AisChainReq {
  const ebm_energy_t& e;
  float* x;                // [n_chains, dim]: the final states, written once
  float* logw;             // [n_chains]
  int64_t n_chains;
  int32_t dim, n_temps, n_leapfrog;
  const float* beta;       // device [n_temps + 1]
  const float* eps;        // device [n_temps]: the step size of every transition
  float sigma0, inv_var0;  // the base N(0, sigma0^2 I)
  uint8_t* accept_mask;
  uint32_t* accept_counts;
  const float* x0;
  const float* p_noise;
  const float* u_accept;
  uint64_t seed, offset;

  RngKey key() const { return RngKey{(uint32_t)seed, (uint32_t)(seed >> 32)}; }
};

struct MomentsChainReq {
  const ebm_energy_t& e;
  float* x;                // [n_chains, dim], in/out
  int64_t n_chains;
  int32_t dim;
  bool hmc;                // the sampler: false = Langevin, true = HMC
  int32_t k_steps, burn_in;
  float eta, sqrt_eta, noise_coef;  // Langevin
  int32_t n_leapfrog;               // HMC
  float eps;
  const float* recip;      // device [half_len()]
  float* mom;              // [4, n_chains, dim]
  float* e_mom;            // [4, n_chains] or null
  float* traj;             // [n_chains, 2 half_len(), dim] or null
  float* e_traj;           // [n_chains, 2 half_len()] or null
  uint8_t* accept_mask;
  uint32_t* accept_count;
  const float* noise_or_p;
  const float* u;
  uint64_t seed, offset;

  RngKey key() const { return RngKey{(uint32_t)seed, (uint32_t)(seed >> 32)}; }
  int32_t half_len() const { return (k_steps - burn_in) / 2; }
};

struct LangevinMomentsChainReq {
  const ebm_energy_t& e;   // the MLP energy
  float* x;                // [n_chains, dim], in/out
  int64_t n_chains;
  int32_t dim, k_steps, burn_in;
  float eta, sqrt_eta, noise_coef;
  const float* recip;      // device [half_len()]
  float* mom;              // [4, n_chains, dim]
  float* e_mom;            // [4, n_chains] or null
  float* traj;             // [n_chains, 2 half_len(), dim] or null
  float* e_traj;           // [n_chains, 2 half_len()] or null
  const float* noise;      // [k_steps, n_chains, dim] or null
  uint64_t seed, offset;

  RngKey key() const { return RngKey{(uint32_t)seed, (uint32_t)(seed >> 32)}; }
  int32_t half_len() const { return (k_steps - burn_in) / 2; }
};

struct KineticChainReq {
  const ebm_energy_t& e;
  float* x;                // [n_chains, dim], in/out
  float* v;                // [n_chains, dim]: in/out, output only with draw_v0
  int64_t n_chains;
  int32_t dim, k_steps;
  float hh, c1, c2, sqrt_temp;  // h / 2, exp(-gamma h), sqrt(T (1 - exp(-2 gamma h))), sqrt(T): formed in double, rounded once
  bool draw_v0;
  int32_t thin;
  float* traj;             // [n_chains, n_kept(), dim] or null
  const float* noise;      // [k_steps, n_chains, dim] or null
  uint64_t seed, offset;

  RngKey key() const { return RngKey{(uint32_t)seed, (uint32_t)(seed >> 32)}; }
  int32_t n_kept() const { return k_steps / thin; }
};

struct GhmcChainReq {
  const ebm_energy_t& e;
  float* x;                // [n_chains, dim], in/out
  float* v;                // [n_chains, dim]: in/out, output only with draw_v0
  int64_t n_chains;
  int32_t dim, n_mh, n_leapfrog;
  // eps, exp(-gamma eps L), sqrt(T (1 - exp(-2 gamma eps L))), sqrt(T), 1 / T: formed in double, rounded once
  float eps, c1, c2, sqrt_temp, beta;
  bool draw_v0;
  int32_t thin;
  float* traj;             // [n_chains, n_kept(), dim] or null
  uint8_t* accept_mask;    // [n_mh, n_chains] or null
  const float* noise;      // [n_mh, n_chains, dim] or null
  const float* u;          // [n_mh, n_chains] or null
  uint64_t seed, offset;

  RngKey key() const { return RngKey{(uint32_t)seed, (uint32_t)(seed >> 32)}; }
  int32_t n_kept() const { return n_mh / thin; }
};

// A scalar or diagonal mass as the massed entries take it (EBM_MASS_SCALAR / EBM_MASS_DIAG; never EBM_MASS_NONE)
struct ChainMass {
  int32_t kind;
  double scalar;      // EBM_MASS_SCALAR: positive and finite
  const float* diag;  // EBM_MASS_DIAG: device [dim]
};

// ebm_kinetic_chain_mass_f32: the unit-mass request, whose v is then the momentum plane, and the mass
struct KineticMassChainReq {
  KineticChainReq chain;
  ChainMass mass;
};

// ebm_ghmc_chain_mass_f32: likewise
struct GhmcMassChainReq {
  GhmcChainReq chain;
  ChainMass mass;
};

struct KineticMomentsChainReq {
  const ebm_energy_t& e;
  float* x;                // [n_chains, dim], in/out
  float* v;                // [n_chains, dim]: in/out, output only with draw_v0
  int64_t n_chains;
  int32_t dim;
  bool ghmc;               // the sampler: false = BAOAB, true = generalized HMC
  int32_t k_steps, burn_in, n_leapfrog;
  // BAOAB: h / 2, exp(-gamma h), sqrt(T (1 - exp(-2 gamma h))); GHMC: eps, exp(-gamma eps L), sqrt(T (1 - exp(-2 gamma eps L))),
  // 1 / T; both: sqrt(T) -- formed in double, rounded once, as the two chain entries form them
  float hh, eps, c1, c2, sqrt_temp, beta;
  bool draw_v0;
  const float* recip;      // device [half_len()]
  float* mom;              // [4, n_chains, dim]
  float* e_mom;            // [4, n_chains] or null
  float* v2_mom;           // [2, n_chains, dim] or null (BAOAB)
  float* traj;             // [n_chains, 2 half_len(), dim] or null
  float* e_traj;           // [n_chains, 2 half_len()] or null
  float* v_traj;           // [n_chains, 2 half_len(), dim] or null (BAOAB)
  uint8_t* accept_mask;    // [k_steps, n_chains] or null (GHMC)
  uint32_t* accept_count;  // [k_steps] or null (GHMC)
  const float* noise;      // [k_steps, n_chains, dim] or null
  const float* u;          // [k_steps, n_chains] or null (GHMC)
  uint64_t seed, offset;

  RngKey key() const { return RngKey{(uint32_t)seed, (uint32_t)(seed >> 32)}; }
  int32_t half_len() const { return (k_steps - burn_in) / 2; }
};

// The fields the row-major Langevin argument structs share (GaussArgs, BigArgs, RowChainArgs, WideArgs).
template <class Args>
inline void fill_langevin(Args& a, const LangevinChainReq& q) {
  a.x = q.x; a.n_chains = q.n_chains; a.dim = q.dim; a.k_steps = q.k_steps;
  a.eta = q.eta; a.sqrt_eta = q.sqrt_eta; a.noise_coef = q.noise_coef;
  a.table = reinterpret_cast<const float4*>(q.coef_table);
  a.clamp_on = q.clamp; a.cmin = q.cmin; a.cmax = q.cmax;
  a.thin = q.thin; a.n_kept = q.n_kept(); a.traj = q.traj; a.noise = q.noise;
  a.key = q.key(); a.step0 = q.offset;
}

// A scalar mass in its three forms: raw (kinetic energy), sqrt (momentum draw), clamped (drift); formed in double, rounded once.
template <class Args>
inline void fill_scalar_mass(Args& a, double m) {
  a.mass_raw = (float)m;
  a.mass_sqrt = (float)sqrt(m);
  a.mass_safe = (float)(m < 1e-10 ? 1e-10 : m);
}

// The mass of the massed kinetic walkers (KineticMassArgs, GhmcMassArgs): the kind, the scalar forms, the diagonal's pointer.
template <class Args>
inline void fill_mass(Args& a, const ChainMass& m) {
  a.mass_kind = m.kind;
  fill_scalar_mass(a, m.kind == EBM_MASS_SCALAR ? m.scalar : 1.0);
  a.mass_diag = m.diag;
}

// The fields the HMC argument structs share (HmcArgs, GaussHmcArgs, WideHmcArgs), the scalar mass in its three forms.
template <class Args>
inline void fill_hmc(Args& a, const HmcChainReq& q) {
  a.x = q.x; a.n_chains = q.n_chains; a.dim = q.dim; a.n_mh = q.n_mh; a.n_leapfrog = q.n_leapfrog;
  a.eps = q.eps; a.eps_table = q.eps_table;
  fill_scalar_mass(a, q.mass_scalar);
  a.thin = q.thin; a.n_kept = q.n_kept(); a.traj = q.traj;
  a.accept_mask = q.accept_mask; a.accept_count = q.accept_count; a.p_noise = q.p_noise; a.u = q.u;
  a.key = q.key(); a.step0 = q.offset;
}

// ---------------------------------------------------------------------------------
// Langevin chain launchers and the predicates that route to them
// ---------------------------------------------------------------------------------
int launch_langevin_chain_elem(const LangevinChainReq&, hipStream_t);       // langevin.hip: double well, harmonic
int launch_langevin_chain_elem_diag(const LangevinChainReq&, hipStream_t);  // langevin_diag.hip: ... with records
bool elem_diag_supported(int32_t dim, bool has_noise, bool has_traj);
bool elem_diag_plan(int64_t n_chains, int32_t dim, diag::DiagArgs&);
int launch_langevin_chain_rows(const LangevinChainReq&, hipStream_t);       // rows_langevin.hip: the lane-group kernels
bool rows_langevin_diag_plan(const ebm_energy_t&, int heun, int64_t n_chains, int32_t dim, diag::DiagArgs&);
int launch_langevin_chain_mlp(const LangevinChainReq&, hipStream_t);        // mlp.hip
int launch_mlp_wide(const LangevinChainReq&, float* energy_out, float* grad_out, hipStream_t, const char* who);  // mlp_wide.hip
bool mlp_wide_supported(int32_t hidden, int32_t dim);
bool mlp_diag_plan(const ebm_energy_t&, bool hmc, int64_t n_chains, int32_t dim, diag::DiagArgs&);
// gauss_mfma.hip: dims 20 .. 128 (multiples of 4), other widths as packed rows, 132 .. 160 with Ps resident in LDS
int launch_langevin_chain_gauss_mfma(const LangevinChainReq&, hipStream_t);
bool gauss_mfma_supported(int32_t dim);
bool gauss_lds5_supported(int32_t dim);
int32_t gauss_pack_factor(int32_t dim, int64_t n_chains);  // 1 as is, > 1 packed rows, 0 no matrix-layout form
int launch_langevin_chain_gmm_mfma(const LangevinChainReq&, hipStream_t);  // gauss_mfma.hip: mixtures up to 32 components
bool gmm_mfma_supported(int32_t dim, int32_t n_comp);
int launch_langevin_chain_matrix_diag(const LangevinChainReq&, hipStream_t);  // gauss_mfma.hip: records of the matrix layout
bool matrix_langevin_diag_plan(const ebm_energy_t&, int64_t n_chains, int32_t dim, diag::DiagArgs&);
int launch_langevin_chain_gauss_shift(const LangevinChainReq&, hipStream_t);  // gauss_shift.hip: widths off multiples of 4, 21 .. 157
bool gauss_shift_supported(int32_t dim);
int launch_langevin_chain_gauss_res_shift(const LangevinChainReq&, hipStream_t);  // gauss_res_shift.hip: ... up to 254, per-class images
bool gauss_res_shift_supported(const ebm_energy_t&, int32_t dim);
int launch_langevin_chain_gauss_big(const LangevinChainReq&, hipStream_t);  // gauss_big.hip: dims 132 .. 512 in steps of 4
bool gauss_big_supported(int32_t dim);
bool gauss_big_diag_plan(int64_t n_chains, int32_t dim, diag::DiagArgs&);
int launch_langevin_chain_gmm_shift(const LangevinChainReq&, hipStream_t);  // gmm_shift.hip: mixtures off multiples of 4, 21 .. 125
bool gmm_shift_supported(int32_t dim, int32_t n_comp);
int launch_langevin_chain_gmm_wide(const LangevinChainReq&, hipStream_t);        // gmm_wide.hip: mixtures at 132 .. 256 dims
int launch_langevin_chain_gmm_wide_shift(const LangevinChainReq&, hipStream_t);  // gmm_wide_shift.hip: ... and the widths between
bool gmm_wide_supported(int32_t dim, int32_t n_comp);
bool gmm_wide_shift_supported(int32_t dim, int32_t n_comp);

// ---------------------------------------------------------------------------------
// HMC chain launchers and the predicates that route to them
// ---------------------------------------------------------------------------------
int launch_hmc_chain(const HmcChainReq&, hipStream_t);        // hmc.hip: routing, then the lane-group kernels
int launch_hmc_chain_audit(const HmcChainReq&, hipStream_t);  // hmc.hip: the literal leapfrog sequence
bool hmc_diag_plan(const ebm_energy_t&, int64_t n_chains, int32_t dim, diag::DiagArgs&);
int launch_hmc_chain_mlp(const HmcChainReq&, hipStream_t);  // mlp.hip
int launch_hmc_chain_mlp_wide(const HmcChainReq&, hipStream_t, const char* who);  // mlp_wide_hmc.hip
bool mlp_wide_hmc_supported(int32_t hidden, int32_t dim);
int launch_hmc_chain_gauss_mfma(const HmcChainReq&, hipStream_t);  // gauss_hmc_mfma.hip: dims 20 .. 160 (multiples of 4)
bool gauss_hmc_mfma_supported(int32_t dim, int32_t mass_kind);
int launch_hmc_chain_gauss_shift(const HmcChainReq&, hipStream_t);       // gauss_hmc_shift.hip: widths off multiples of 4, 17 .. 158
int launch_hmc_chain_gauss_shift_diag(const HmcChainReq&, hipStream_t);  // gauss_hmc_shift_diag.hip: ... with records
bool gauss_hmc_shift_supported(int32_t dim);
int launch_hmc_chain_gauss_stream(const HmcChainReq&, hipStream_t);  // gauss_hmc_stream.hip: dims 164 .. 256 with the pre-split image
bool gauss_hmc_stream_supported(const ebm_energy_t&, int32_t dim);
int launch_hmc_chain_gauss_stream_shift(const HmcChainReq&, hipStream_t);       // gauss_hmc_stream_shift.hip: ... the widths between
int launch_hmc_chain_gauss_stream_shift_diag(const HmcChainReq&, hipStream_t);  // gauss_hmc_stream_shift_diag.hip: ... with records
bool gauss_hmc_stream_shift_supported(const ebm_energy_t&, int32_t dim);
int launch_hmc_chain_gmm_mfma(const HmcChainReq&, hipStream_t);  // gmm_hmc_mfma.hip: mixtures up to 32 components, dims up to 128
bool gmm_hmc_mfma_supported(int32_t dim, int32_t n_comp, int32_t mass_kind);
int launch_hmc_chain_gmm_shift(const HmcChainReq&, hipStream_t);       // gmm_hmc_shift.hip: mixtures off multiples of 4
int launch_hmc_chain_gmm_shift_diag(const HmcChainReq&, hipStream_t);  // gmm_hmc_shift_diag.hip: ... with records
bool gmm_hmc_shift_supported(int32_t dim, int32_t n_comp, int32_t mass_kind, bool records);
int launch_hmc_chain_gmm_wide(const HmcChainReq&, hipStream_t);        // gmm_hmc_wide.hip: mixtures at 132 .. 224 dims
int launch_hmc_chain_gmm_wide_shift(const HmcChainReq&, hipStream_t);  // gmm_hmc_wide_shift.hip: ... and the widths between
bool gmm_hmc_wide_supported(int32_t dim, int32_t n_comp, int32_t mass_kind);
bool gmm_hmc_wide_shift_supported(int32_t dim, int32_t n_comp, int32_t mass_kind);
int launch_hmc_chain_matrix_diag(const HmcChainReq&, hipStream_t);  // matrix_hmc_diag.hip: records of the matrix layout
bool matrix_hmc_diag_plan(const ebm_energy_t&, int64_t n_chains, int32_t dim, diag::DiagArgs&);

// ---------------------------------------------------------------------------------
// The walks on the wide MLP energy (mlp_wide_*.hip; the ... on the MLP energy launchers below)
// ---------------------------------------------------------------------------------
// Which MLP shapes the fused walks take, said once: 0, or the refusal under the entry's name `who` (hidden width not 64 / 128,
// dim outside 1 .. 128).  No launch and no device access: an entry calls it in front of its early return for an empty call, so
// it needs no GPU; the launcher calls it again.  (samplers/_chain_host.py, fused_mlp_walk_fits, is the Python form.)
inline int wide_mlp_check_shape(const char* who, int32_t hidden, int32_t dim) {
  if ((hidden != 64 && hidden != 128) || dim < 1 || dim > 128)
    return fail(EBM_EDIM, "%s: the fused MLP walk supports hidden width 64 or 128 and 1 <= dim <= 128 (got %d, %d)", who, hidden, dim);
  return 0;
}
// ... of the tempered walks, whose waves hold whole ladders: and n_replicas not in {2, 4, 8, 16, 32}
inline int wide_mlp_check_ladder_shape(const char* who, int32_t hidden, int32_t dim, int32_t n_replicas) {
  const bool ladder_ok = n_replicas == 2 || n_replicas == 4 || n_replicas == 8 || n_replicas == 16 || n_replicas == 32;
  if ((hidden != 64 && hidden != 128) || dim < 1 || dim > 128 || !ladder_ok)
    return fail(EBM_EDIM,
                "%s: the fused MLP ladder supports hidden width 64 or 128, 1 <= dim <= 128 and 2, 4, 8, 16 or 32 replicas "
                "(got %d, %d, %d)",
                who, hidden, dim, n_replicas);
  return 0;
}

// ---------------------------------------------------------------------------------
// Replica-exchange Langevin (tempering.hip: a ladder of tempered walkers per chain, swaps inside the launch)
// ---------------------------------------------------------------------------------
int tempering_chain_launch(const TemperingChainReq&, hipStream_t);
int tempering_check_geometry(int32_t n_replicas, int32_t dim);  // 0, or the refusal (dim > 1024, ladder wider than a workgroup)
// ... on the MLP energy (mlp_wide_tempering_langevin.hip: the same request; 32 slot rows per wave around the matrix-core evaluation, one per step, a swap moves state and gradient between neighbouring lanes)
int tempering_mlp_chain_launch(const TemperingChainReq&, hipStream_t);

// ---------------------------------------------------------------------------------
// Replica-exchange HMC (tempering_hmc.hip: the same ladders, a Metropolis-corrected HMC transition in every slot)
// ---------------------------------------------------------------------------------
int tempering_hmc_chain_launch(const TemperingHmcChainReq&, hipStream_t);
int tempering_hmc_check_geometry(int32_t n_replicas, int32_t dim);  // 0, or the refusal (dim > 256, ladder wider than a workgroup)
// ... on the MLP energy (mlp_wide_tempering.hip: the same request; 32 slot rows per wave around the matrix-core evaluation, n_leapfrog + 1 of them per transition, a swap moves the states between neighbouring lanes)
int tempering_hmc_mlp_chain_launch(const TemperingHmcChainReq&, hipStream_t);

// ---------------------------------------------------------------------------------
// Annealed importance sampling (ais.hip: one walker per chain through the temperatures in time, the weight from carried energies)
// ---------------------------------------------------------------------------------
int ais_chain_launch(const AisChainReq&, hipStream_t);
int ais_check_geometry(int32_t dim);  // 0, or the refusal (dim > 256)
// ... on the MLP energy (mlp_wide_ais.hip: the same request; 32 chains per wave around the matrix-core evaluation, n_leapfrog + 1 of them per transition)
int ais_mlp_chain_launch(const AisChainReq&, hipStream_t);


// ---------------------------------------------------------------------------------
// Per-chain running moments (moments.hip: a Langevin or an HMC walker per chain with Welford pairs beside the state)
// ---------------------------------------------------------------------------------
int moments_chain_launch(const MomentsChainReq&, hipStream_t);
int moments_check_geometry(int32_t dim);  // 0, or the refusal (dim > 256)
// ... of the Langevin walker on the MLP energy (mlp_wide_langevin_moments.hip: 32 chains per wave around the matrix-core evaluation, k_steps of them per call and one more with energies, the Welford pairs kept in the caller's planes)
int langevin_moments_mlp_chain_launch(const LangevinMomentsChainReq&, hipStream_t);

// ---------------------------------------------------------------------------------
// Underdamped Langevin, BAOAB (kinetic.hip: a walker per chain with position, velocity and carried gradient in registers)
// ---------------------------------------------------------------------------------
int kinetic_chain_launch(const KineticChainReq&, hipStream_t);
int kinetic_check_geometry(int32_t dim);  // 0, or the refusal (dim > 256)
// ... on the MLP energy (mlp_wide_kinetic.hip: the same request; 32 chains per wave around the matrix-core evaluation, k_steps + 1 of them per call)
int kinetic_mlp_chain_launch(const KineticChainReq&, hipStream_t);

// ---------------------------------------------------------------------------------
// Generalized HMC (ghmc.hip: the kinetic walker with a partial momentum refresh, a Metropolis-corrected trajectory and the flip)
// ---------------------------------------------------------------------------------
int ghmc_chain_launch(const GhmcChainReq&, hipStream_t);
int ghmc_check_geometry(int32_t dim);  // 0, or the refusal (dim > 256)
// ... on the MLP energy (mlp_wide_ghmc.hip: the same request; 32 chains per wave around the matrix-core evaluation, n_leapfrog + 1 of them per transition)
int ghmc_mlp_chain_launch(const GhmcChainReq&, hipStream_t);

// ---------------------------------------------------------------------------------
// The two with a scalar or diagonal mass (kinetic_mass.hip, ghmc_mass.hip: the same walkers, the carried plane the momentum)
// ---------------------------------------------------------------------------------
int kinetic_mass_chain_launch(const KineticMassChainReq&, hipStream_t);
int ghmc_mass_chain_launch(const GhmcMassChainReq&, hipStream_t);
// ... on the MLP energy (mlp_wide_kinetic_mass.hip, mlp_wide_ghmc_mass.hip: the same requests; the walks of the two MLP entries above, the mass forms in LDS tables read a register quad at a time)
int kinetic_mass_mlp_chain_launch(const KineticMassChainReq&, hipStream_t);
int ghmc_mass_mlp_chain_launch(const GhmcMassChainReq&, hipStream_t);

// ---------------------------------------------------------------------------------
// Running moments of the two (kinetic_moments.hip: the BAOAB or the GHMC walker with Welford pairs beside position and velocity)
// ---------------------------------------------------------------------------------
int kinetic_moments_chain_launch(const KineticMomentsChainReq&, hipStream_t);
int kinetic_moments_check_geometry(int32_t dim);  // 0, or the refusal (dim outside 1 .. 256)
// ... on the MLP energy (mlp_wide_kinetic_moments.hip, mlp_wide_ghmc_moments.hip: the same request; the walks of the two MLP entries above with the Welford pairs kept in the caller's planes, updated in place once per counted transition)
int kinetic_moments_mlp_chain_launch(const KineticMomentsChainReq&, hipStream_t);

}  // namespace ebm
