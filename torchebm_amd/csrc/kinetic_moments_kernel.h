// Per-chain running moments of the two velocity-carrying samplers: the BAOAB walker of kinetic_kernel.h and the generalized-HMC
// walker of ghmc_kernel.h, each with the Welford pairs of moments_kernel.h (moments::Accum / welford, reused, not copied)
// beside position and velocity, in registers from the load to the one store (ebm_kinetic_moments_f32, include/ebm_hip.h;
// docs/design/kinetic_moments.md).
//
// Layout: rows.h -- a lane group is a chain.  BAOAB: x, v, g (12 registers), the coordinate pairs (16), the energy pairs (4)
// and the running mean of v^2 of both halves (8).  GHMC: xc, v, the carried force and the transition's temporaries, the
// coordinate and energy pairs.  A chain never talks to another: no exchange, no barrier in the loop beyond what Energy::eval
// needs; recip[c - 1], the burn-in test and the half switch are wave-uniform, and the half switch is taken once per launch
// (next_half_*), not selected per step.
//
// Transitions: kinetic_chain's recurrence and ghmc_chain's transition, operation for operation; what is counted is the state
// behind the transition.  BAOAB with energies takes E of the post-step position out of the one evaluation inside the step
// (eval<true>): that position is the counted state, so nothing is pending and nothing is evaluated behind the loop.
#pragma once
#include "moments_kernel.h"

namespace ebm {
namespace kinetic_moments {
using namespace rows;

struct KineticMomentsArgs {
  float* x;                // [n_chains, dim], in/out
  float* v;                // [n_chains, dim]: in/out, output only with draw_v0
  int64_t n_chains;
  int32_t dim, k_steps, burn_in, half_len, n_leapfrog, draw_v0;
  float hh;                // BAOAB: h / 2
  float eps, beta;         // GHMC
  float c1, c2, sqrt_temp;
  const float* recip;      // device [half_len]: float32(1 / c), c = 1 .. half_len
  float* mom;              // [4, n_chains, dim]: mean_a, M2_a, mean_b, M2_b
  float* e_mom;            // [4, n_chains] or null
  float* v2_mom;           // [2, n_chains, dim] or null (BAOAB): the mean of v^2 of either half
  float* traj;             // [n_chains, 2 half_len, dim] or null
  float* e_traj;           // [n_chains, 2 half_len] or null
  float* v_traj;           // [n_chains, 2 half_len, dim] or null (BAOAB)
  uint8_t* accept_mask;    // [k_steps, n_chains] or null (GHMC)
  uint32_t* accept_count;  // [k_steps] or null (GHMC)
  const float* noise;      // [k_steps, n_chains, dim] or null
  const float* u;          // [k_steps, n_chains] or null (GHMC)
  RngKey key;
  uint64_t step0;
  EnergyParams energy;
  int param_floats;
};

// the fields moments::Accum::store reads
__device__ __forceinline__ moments::MomentsArgs store_args(const KineticMomentsArgs& a) {
  moments::MomentsArgs m{};
  m.n_chains = a.n_chains;
  m.dim = a.dim;
  m.mom = a.mom;
  m.e_mom = a.e_mom;
  return m;
}

namespace {

extern __shared__ __attribute__((aligned(16))) float kinetic_moments_smem[];

// ---- BAOAB.  WANT_E: the evaluation inside the step returns the energy of the post-step position beside the gradient;
//      without it no step carries a group reduction.
template <int KIND, int G, bool FULL, bool WANT_E>
__device__ __forceinline__ void baoab_body(const KineticMomentsArgs& a) {
  using LaneT = Lane<G, 1, FULL>;
  LaneT L;
  L.init(a.n_chains, a.dim);
  const Smem S = carve_smem<1>(kinetic_moments_smem, a.param_floats);
  stage_params(a.energy, a.dim, S.param);
  Energy<KIND, LaneT> en;
  en.init(a.energy, L, S);

  const int64_t row = L.active ? L.chain * (int64_t)a.dim : 0;
  const bool leader = L.active && L.lg == 0;
  const int64_t traj_row = L.active ? L.chain * (2 * (int64_t)a.half_len) * a.dim : 0;
  const int64_t e_row = L.active ? L.chain * (2 * (int64_t)a.half_len) : 0;
  const float hh = a.hh, c1 = a.c1, c2 = a.c2;
  Slice<1> x, v, g;
  load_slice(L, a.x, row, x);
  if (a.draw_v0) {  // wave-uniform
    normal_slice(L, a.key, a.step0, v);
#pragma unroll
    for (int i = 0; i < 4; ++i) v.a[0][i] = L.ok(0, i) ? a.sqrt_temp * v.a[0][i] : 0.0f;
  } else {
    load_slice(L, a.v, row, v);
  }
  moments::Accum<LaneT> acc;
  acc.zero();
  Slice<1> v2_a, v2_b;  // the running mean of v^2, first half and the half being filled
#pragma unroll
  for (int i = 0; i < 4; ++i) v2_a.a[0][i] = v2_b.a[0][i] = 0.0f;
  en.template eval<false>(L, x, g);  // the raw gradient, no clamp: a NaN stays in its chain

  for (int s = 0; s < a.k_steps; ++s) {
    Slice<1> xi;
    if (a.noise) load_slice(L, a.noise, ((int64_t)s * a.n_chains) * a.dim + row, xi);
    else normal_slice(L, a.key, a.step0 + 1ull + (uint64_t)s, xi);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      // B, A, O, A: every operation rounded on its own
      float vi = v.a[0][i] - hh * g.a[0][i];
      float xv = x.a[0][i] + hh * vi;
      vi = c1 * vi + c2 * xi.a[0][i];
      xv = xv + hh * vi;
      x.a[0][i] = L.ok(0, i) ? xv : 0.0f;
      v.a[0][i] = L.ok(0, i) ? vi : 0.0f;
    }
    const float e = en.template eval<WANT_E>(L, x, g);
#pragma unroll
    for (int i = 0; i < 4; ++i) {  // B
      const float vi = v.a[0][i] - hh * g.a[0][i];
      v.a[0][i] = L.ok(0, i) ? vi : 0.0f;
    }
    if (s >= a.burn_in) {  // wave-uniform
      const int j = s - a.burn_in;
      const bool second = j >= a.half_len;
      const float rc = a.recip[second ? j - a.half_len : j];  // wave-uniform load
      if (j == a.half_len) {
        acc.next_half_state();
        if constexpr (WANT_E) acc.next_half_energy();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          v2_a.a[0][i] = v2_b.a[0][i];
          v2_b.a[0][i] = 0.0f;
        }
      }
      acc.add_state(x, rc);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float vv = v.a[0][i] * v.a[0][i];
        v2_b.a[0][i] = v2_b.a[0][i] + (vv - v2_b.a[0][i]) * rc;
      }
      if (a.traj) store_slice(L, a.traj, traj_row + (int64_t)j * a.dim, x);
      if (a.v_traj) store_slice(L, a.v_traj, traj_row + (int64_t)j * a.dim, v);
      if constexpr (WANT_E) {
        acc.add_energy(e, rc);
        if (a.e_traj && leader) a.e_traj[e_row + j] = e;
      }
    }
  }
  store_slice(L, a.x, row, x);
  store_slice(L, a.v, row, v);
  acc.store(L, store_args(a), row, leader, WANT_E);
  if (a.v2_mom) {  // wave-uniform
    store_slice(L, a.v2_mom, row, v2_a);
    store_slice(L, a.v2_mom, a.n_chains * (int64_t)a.dim + row, v2_b);
  }
}

template <int KIND, int G, int NV, bool FULL>
__global__ __launch_bounds__(kBlock) void moments_kinetic_chain(KineticMomentsArgs a) {
  static_assert(NV == 1, "one vector per lane");
  baoab_body<KIND, G, FULL, false>(a);
}

template <int KIND, int G, int NV, bool FULL>
__global__ __launch_bounds__(kBlock) void moments_kinetic_chain_energy(KineticMomentsArgs a) {
  static_assert(NV == 1, "one vector per lane");
  baoab_body<KIND, G, FULL, true>(a);
}

// ---- GHMC: ghmc_chain's transition; the energy of a counted state is the one the transition carries.
template <int KIND, int G, int NV, bool FULL>
__global__ __launch_bounds__(kBlock) void moments_ghmc_chain(KineticMomentsArgs a) {
  static_assert(NV == 1, "one vector per lane");
  using LaneT = Lane<G, 1, FULL>;
  LaneT L;
  L.init(a.n_chains, a.dim);
  const Smem S = carve_smem<1>(kinetic_moments_smem, a.param_floats);
  stage_params(a.energy, a.dim, S.param);
  Energy<KIND, LaneT> en;
  en.init(a.energy, L, S);

  const int64_t row = L.active ? L.chain * (int64_t)a.dim : 0;
  const bool leader = L.active && L.lg == 0;
  const int64_t traj_row = L.active ? L.chain * (2 * (int64_t)a.half_len) * a.dim : 0;
  const int64_t e_row = L.active ? L.chain * (2 * (int64_t)a.half_len) : 0;
  const float c1 = a.c1, c2 = a.c2, beta = a.beta;
  Slice<1> xc, v;
  load_slice(L, a.x, row, xc);
  if (a.draw_v0) {  // wave-uniform
    normal_slice(L, a.key, a.step0, v);
#pragma unroll
    for (int i = 0; i < 4; ++i) v.a[0][i] = L.ok(0, i) ? a.sqrt_temp * v.a[0][i] : 0.0f;
  } else {
    load_slice(L, a.v, row, v);
  }
  moments::Accum<LaneT> acc;
  acc.zero();
  const bool with_energy = a.e_mom != nullptr;

  const hmc::IdentityKinetic<LaneT> kinetic{L};

  // energy and clamped force of the held state, carried; those of the start come out of the pseudo-transition t = -1
  // (hmc_kernel.h), which leaves v alone
  Slice<1> f;
#pragma unroll
  for (int i = 0; i < 4; ++i) f.a[0][i] = 0.0f;
  float e_cur = 0.0f;

  for (int t = -1; t < a.k_steps; ++t) {
    const bool init = t < 0;
    const float eps_t = init ? 0.0f : a.eps;
    const float half_eps = 0.5f * eps_t;

    // ---- O: the partial refresh, two products and a sum, each rounded on its own
    Slice<1> p;
    if (init) {
#pragma unroll
      for (int i = 0; i < 4; ++i) p.a[0][i] = 0.0f;
    } else {
      Slice<1> xi;
      if (a.noise) load_slice(L, a.noise, ((int64_t)t * a.n_chains) * a.dim + row, xi);
      else normal_slice(L, a.key, a.step0 + 1ull + 2ull * (uint64_t)t, xi);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float vo = c1 * v.a[0][i] + c2 * xi.a[0][i];
        p.a[0][i] = L.ok(0, i) ? vo : 0.0f;
      }
    }
    const Slice<1> v_o = p;  // the velocity after O: a reject hands back its negative

    // ---- the accept uniform of this chain, drawn in front of the trajectory as in ghmc_chain
    float uu;
    if (init) uu = -1.0f;
    else if (a.u) uu = L.active ? a.u[(int64_t)t * a.n_chains + L.chain] : 2.0f;
    else uu = u01_half_open(pick(philox_at(a.key, (uint64_t)L.chain >> 2, a.step0 + 2ull + 2ull * (uint64_t)t),
                                 (int)(L.chain & 3)));

    // ---- H0 from the carried energy
    const float e0 = e_cur;
    const float h0 = clamp_nanprop(e0, -1e10f, 1e10f) + kinetic(p);

    // ---- proposal
    const Slice<1> f_keep = f;
    Slice<1> x = xc;
    const int n_lf = init ? 1 : a.n_leapfrog;
    const float e1 = hmc::leapfrog_steps<false>(en, L, x, p, f, x, eps_t, half_eps, n_lf, e0, init);
    const float h1 = clamp_nanprop(e1, -1e10f, 1e10f) + kinetic(p);

    // ---- Metropolis accept at the temperature T
    const bool accept = hmc::metropolis_accept(beta * (h0 - h1), uu, init, L.active);
    if (accept) {
      e_cur = e1;
      xc = x;
    } else {
      f = f_keep;
    }
    if (init) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i) v.a[0][i] = accept ? p.a[0][i] : -v_o.a[0][i];  // the flip

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
  store_slice(L, a.v, row, v);
  acc.store(L, store_args(a), row, leader, with_energy);
}

}  // namespace

// The launchers of one energy kind: defined and instantiated in kinetic_moments_unit.hip (one object per kind and sampler).
template <int KIND>
void launch_baoab_kind(const Geometry& geo, dim3 grid, size_t smem, hipStream_t st, const KineticMomentsArgs& a);
template <int KIND>
void launch_ghmc_kind(const Geometry& geo, dim3 grid, size_t smem, hipStream_t st, const KineticMomentsArgs& a);

}  // namespace kinetic_moments
}  // namespace ebm
