// Per-chain running moments: a Langevin walker and an HMC walker that keep, beside the state, a Welford pair per coordinate
// and per half of the counted steps -- and one for the energy -- in registers, and store them once
// (ebm_chain_moments_f32, include/ebm_hip.h; docs/design/moments.md).
//
// Layout: rows.h -- a lane group is a chain that keeps its state and its accumulators in registers from the load to the one
// store at the end: 16 registers for the coordinates (mean, M2 of both halves), 4 for the energy.  A chain never talks to
// another: no exchange, no barrier in the loop; recip[c - 1], the half switch and the burn-in test are wave-uniform.
//
// Transitions: the Euler-Maruyama step of rows_langevin.hip / tempering_kernel.h in the reference's op order, and
// hmc_chain_body's transition (hmc_kernel.h: leapfrog_steps<false>, IdentityKinetic, metropolis_accept; the draws spelled as
// hmc_chain_body spells them) with energy and force carried from the accepted state, the start's from the pseudo-transition.
#pragma once
#include "chain_launch.h"
#include "hmc_kernel.h"
#include "landscape_energies.h"

namespace ebm {
namespace moments {
using namespace rows;

struct MomentsArgs {
  float* x;                // [n_chains, dim], in/out
  int64_t n_chains;
  int32_t dim, k_steps, burn_in, half_len, n_leapfrog;
  float eta, sqrt_eta, noise_coef;  // Langevin
  float eps;                        // HMC
  const float* recip;      // device [half_len]: float32(1 / c), c = 1 .. half_len
  float* mom;              // [4, n_chains, dim]: mean_a, M2_a, mean_b, M2_b
  float* e_mom;            // [4, n_chains] or null
  float* traj;             // [n_chains, 2 half_len, dim] or null
  float* e_traj;           // [n_chains, 2 half_len] or null
  uint8_t* accept_mask;    // [k_steps, n_chains] or null (HMC)
  uint32_t* accept_count;  // [k_steps] or null (HMC)
  const float* noise;      // Langevin: [k_steps, n_chains, dim]; HMC: the momenta, same shape; or null
  const float* u;          // HMC: [k_steps, n_chains] or null
  RngKey key;
  uint64_t step0;
  EnergyParams energy;
  int param_floats;
};

// One Welford step, every operation rounded on its own (the units compile with -ffp-contract=off): rc = recip[c - 1].
// From zeros, c = 1 gives mean = x and M2 = 0 with no special case.
__device__ __forceinline__ void welford(float& mean, float& m2, float x, float rc) {
  const float d = x - mean;
  mean = mean + d * rc;
  m2 = m2 + d * (x - mean);
}

// The accumulators of one chain: both halves of the coordinates, both halves of the energy.  Every step adds to the b pairs;
// when the first half is full they move to the a pairs and start again from zero (next_half_*(), wave-uniform, once per
// launch), so the loop selects nothing and addresses no register through a pointer.
template <class LaneT>
struct Accum {
  Slice<1> mean_a, m2_a, mean_b, m2_b;
  float e_mean_a, e_m2_a, e_mean_b, e_m2_b;

  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int i = 0; i < 4; ++i) mean_a.a[0][i] = m2_a.a[0][i] = mean_b.a[0][i] = m2_b.a[0][i] = 0.0f;
    e_mean_a = e_m2_a = e_mean_b = e_m2_b = 0.0f;
  }
  __device__ __forceinline__ void add_state(const Slice<1>& x, float rc) {
#pragma unroll
    for (int i = 0; i < 4; ++i) welford(mean_b.a[0][i], m2_b.a[0][i], x.a[0][i], rc);
  }
  __device__ __forceinline__ void add_energy(float e, float rc) { welford(e_mean_b, e_m2_b, e, rc); }
  __device__ __forceinline__ void next_half_state() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      mean_a.a[0][i] = mean_b.a[0][i];
      m2_a.a[0][i] = m2_b.a[0][i];
      mean_b.a[0][i] = m2_b.a[0][i] = 0.0f;
    }
  }
  __device__ __forceinline__ void next_half_energy() {
    e_mean_a = e_mean_b;
    e_m2_a = e_m2_b;
    e_mean_b = e_m2_b = 0.0f;
  }
  // the one store: slots of a lane that hold no column never reach memory (store_slice)
  __device__ __forceinline__ void store(const LaneT& L, const MomentsArgs& a, int64_t row, bool leader, bool with_energy) const {
    const int64_t plane = a.n_chains * (int64_t)a.dim;
    store_slice(L, a.mom, row, mean_a);
    store_slice(L, a.mom, plane + row, m2_a);
    store_slice(L, a.mom, 2 * plane + row, mean_b);
    store_slice(L, a.mom, 3 * plane + row, m2_b);
    if (with_energy && leader) {
      a.e_mom[L.chain] = e_mean_a;
      a.e_mom[a.n_chains + L.chain] = e_m2_a;
      a.e_mom[2 * a.n_chains + L.chain] = e_mean_b;
      a.e_mom[3 * a.n_chains + L.chain] = e_m2_b;
    }
  }
};

namespace {

extern __shared__ __attribute__((aligned(16))) float moments_smem[];

// ---- Langevin.  WANT_E: the energy of a counted state comes out of the evaluation at the top of the NEXT step (energy and
//      gradient together), the last one's out of one evaluation behind the loop; without it no step carries a group reduction.
template <int KIND, int G, bool FULL, bool WANT_E>
__device__ __forceinline__ void langevin_body(const MomentsArgs& a) {
  using LaneT = Lane<G, 1, FULL>;
  LaneT L;
  L.init(a.n_chains, a.dim);
  const Smem S = carve_smem<1>(moments_smem, a.param_floats);
  stage_params(a.energy, a.dim, S.param);
  Energy<KIND, LaneT> en;
  en.init(a.energy, L, S);

  const int64_t row = L.active ? L.chain * (int64_t)a.dim : 0;
  const bool leader = L.active && L.lg == 0;
  const int64_t traj_row = L.active ? L.chain * (2 * (int64_t)a.half_len) * a.dim : 0;
  const int64_t e_row = L.active ? L.chain * (2 * (int64_t)a.half_len) : 0;
  Slice<1> x;
  load_slice(L, a.x, row, x);
  Accum<LaneT> acc;
  acc.zero();
  const float eta = a.eta, sqrt_eta = a.sqrt_eta, noise_coef = a.noise_coef;
  // the slot of the state counted last: its energy is known one evaluation later
  bool pend = false;
  float pend_rc = 0.0f;
  int pend_j = 0;

  for (int s = 0; s < a.k_steps; ++s) {
    Slice<1> g, eps;
    const float e = en.template eval<WANT_E>(L, x, g);
    if constexpr (WANT_E) {
      if (pend) {  // wave-uniform
        if (pend_j == a.half_len) acc.next_half_energy();
        acc.add_energy(e, pend_rc);
        if (a.e_traj && leader) a.e_traj[e_row + pend_j] = e;
      }
    }
    if (a.noise) load_slice(L, a.noise, ((int64_t)s * a.n_chains) * a.dim + row, eps);
    else normal_slice(L, a.key, a.step0 + (uint64_t)s, eps);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      // the reference's op order, as rows_langevin.hip: rounded mul, rounded add
      const float x1 = x.a[0][i] - eta * g.a[0][i];
      const float dw = eps.a[0][i] * sqrt_eta;
      const float nv = x1 + noise_coef * dw;
      x.a[0][i] = L.ok(0, i) ? nv : 0.0f;
    }
    if (s >= a.burn_in) {  // wave-uniform
      const int j = s - a.burn_in;
      const bool second = j >= a.half_len;
      const float rc = a.recip[second ? j - a.half_len : j];  // wave-uniform load
      if (j == a.half_len) acc.next_half_state();
      acc.add_state(x, rc);
      if (a.traj) store_slice(L, a.traj, traj_row + (int64_t)j * a.dim, x);
      pend = true; pend_rc = rc; pend_j = j;
    }
  }
  if constexpr (WANT_E) {
    if (pend) {
      Slice<1> g;
      const float e = en.template eval<true>(L, x, g);
      acc.add_energy(e, pend_rc);
      if (a.e_traj && leader) a.e_traj[e_row + pend_j] = e;
    }
  }
  store_slice(L, a.x, row, x);
  acc.store(L, a, row, leader, WANT_E);
}

template <int KIND, int G, int NV, bool FULL>
__global__ __launch_bounds__(kBlock) void moments_langevin_chain(MomentsArgs a) {
  static_assert(NV == 1, "one vector per lane");
  langevin_body<KIND, G, FULL, false>(a);
}

template <int KIND, int G, int NV, bool FULL>
__global__ __launch_bounds__(kBlock) void moments_langevin_chain_energy(MomentsArgs a) {
  static_assert(NV == 1, "one vector per lane");
  langevin_body<KIND, G, FULL, true>(a);
}

// ---- HMC: hmc_chain_body's transition (identity mass, one vector per lane, state and force in registers); the energy of a
//      counted state is the one the transition carries.
template <int KIND, int G, int NV, bool FULL>
__global__ __launch_bounds__(kBlock) void moments_hmc_chain(MomentsArgs a) {
  static_assert(NV == 1, "one vector per lane");
  using LaneT = Lane<G, NV, FULL>;
  LaneT L;
  L.init(a.n_chains, a.dim);
  const Smem S = carve_smem<NV>(moments_smem, a.param_floats);
  stage_params(a.energy, a.dim, S.param);
  Energy<KIND, LaneT> en;
  en.init(a.energy, L, S);

  const int64_t row = L.active ? L.chain * (int64_t)a.dim : 0;
  const bool leader = L.active && L.lg == 0;
  const int64_t traj_row = L.active ? L.chain * (2 * (int64_t)a.half_len) * a.dim : 0;
  const int64_t e_row = L.active ? L.chain * (2 * (int64_t)a.half_len) : 0;
  Slice<NV> xc;  // current (accepted) state
  load_slice(L, a.x, row, xc);
  Accum<LaneT> acc;
  acc.zero();
  const bool with_energy = a.e_mom != nullptr;

  const hmc::IdentityKinetic<LaneT> kinetic{L};

  // energy and clamped force of the held state, carried; those of the start come out of the pseudo-transition t = -1
  // (hmc_kernel.h: zero momentum, zero step size, one leapfrog step, always taken), so the energy is inlined at one call site
  Slice<NV> f;
#pragma unroll
  for (int i = 0; i < 4; ++i) f.a[0][i] = 0.0f;
  float e_cur = 0.0f;

  for (int t = -1; t < a.k_steps; ++t) {
    const bool init = t < 0;
    const float eps_t = init ? 0.0f : a.eps;
    const float half_eps = 0.5f * eps_t;

    // ---- momentum draw
    Slice<NV> p;
    if (init) {
#pragma unroll
      for (int i = 0; i < 4; ++i) p.a[0][i] = 0.0f;
    } else {
      if (a.noise) load_slice(L, a.noise, ((int64_t)t * a.n_chains) * a.dim + row, p);
      else normal_slice(L, a.key, a.step0 + 2ull * (uint64_t)t, p);
#pragma unroll
      for (int i = 0; i < 4; ++i) p.a[0][i] = L.ok(0, i) ? p.a[0][i] : 0.0f;
    }

    // ---- the accept uniform, drawn in front of the trajectory as in hmc_chain_body
    float uu;
    if (init) uu = -1.0f;
    else if (a.u) uu = L.active ? a.u[(int64_t)t * a.n_chains + L.chain] : 2.0f;
    else uu = u01_half_open(pick(philox_at(a.key, (uint64_t)L.chain >> 2, a.step0 + 2ull * (uint64_t)t + 1ull),
                                 (int)(L.chain & 3)));

    // ---- H0 from the carried energy
    const float e0 = e_cur;
    const float h0 = clamp_nanprop(e0, -1e10f, 1e10f) + kinetic(p);

    // ---- proposal
    Slice<NV> f_keep = f;
    Slice<NV> x = xc;
    const int n_lf = init ? 1 : a.n_leapfrog;
    const float e1 = hmc::leapfrog_steps<false>(en, L, x, p, f, x, eps_t, half_eps, n_lf, e0, init);
    const float h1 = clamp_nanprop(e1, -1e10f, 1e10f) + kinetic(p);

    // ---- Metropolis accept
    const bool accept = hmc::metropolis_accept(h0 - h1, uu, init, L.active);
    if (accept) {
      xc = x;
      e_cur = e1;
    } else {
      f = f_keep;
    }
    if (init) continue;

    if (a.accept_mask && leader) a.accept_mask[(int64_t)t * a.n_chains + L.chain] = accept ? 1 : 0;
    if (a.accept_count) {  // one ballot and one atomic per wave and transition
      const unsigned long long b = __ballot(accept && leader);
      if ((threadIdx.x & 63) == 0 && b) atomicAdd(a.accept_count + t, (uint32_t)__popcll(b));
    }

    if (t >= a.burn_in) {  // wave-uniform; a rejected proposal counts the held state again
      const int j = t - a.burn_in;
      const bool second = j >= a.half_len;
      const float rc = a.recip[second ? j - a.half_len : j];  // wave-uniform load
      if (j == a.half_len) {
        acc.next_half_state();
        acc.next_half_energy();
      }
      acc.add_state(xc, rc);
      acc.add_energy(e_cur, rc);
      if (a.traj) store_slice(L, a.traj, traj_row + (int64_t)j * a.dim, xc);
      if (a.e_traj && leader) a.e_traj[e_row + j] = e_cur;
    }
  }
  store_slice(L, a.x, row, xc);
  acc.store(L, a, row, leader, with_energy);
}

}  // namespace

// The launchers of one energy kind: defined and instantiated in moments_unit.hip (one object per kind and sampler).
template <int KIND>
void launch_langevin_kind(const Geometry& geo, dim3 grid, size_t smem, hipStream_t st, const MomentsArgs& a);
template <int KIND>
void launch_hmc_kind(const Geometry& geo, dim3 grid, size_t smem, hipStream_t st, const MomentsArgs& a);

}  // namespace moments
}  // namespace ebm
