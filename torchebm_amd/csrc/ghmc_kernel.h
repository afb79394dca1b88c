// Generalized HMC (Horowitz 1991; Metropolis-adjusted kinetic Langevin): a walker per chain that keeps position, velocity, the
// carried energy and the carried clamped force in registers from the load to the one store.  ONE walker, `walk`, behind three
// entries (docs/design/ghmc.md, adapt.md, adapt_mass.md):
//
//   kernel                  entry                            mass     step size
//   ghmc_chain              ebm_ghmc_chain_f32               unit     fixed
//   ghmc_adapt_chain        ebm_ghmc_adapt_chain_f32         unit     dual averaging (Hoffman & Gelman 2014, section 3.2; Stan's
//   ghmc_adapt_mass_chain   ebm_ghmc_adapt_chain_mass_f32    massed   shape: every chain adapts its own step size from its alpha)
//
// The fourth combination, massed with a fixed step (ghmc_mass_chain, ebm_ghmc_chain_mass_f32), stays a kernel of its own in
// ghmc_mass_kernel.h: instantiated from this walker it computes the same bits, but its masked Gaussian rows at G = 32 take 169
// VGPRs instead of 167 and lose a wave, with the body behind any function at all.
//
// The two axes are compile-time policies keyed by the part of the argument struct that carries their fields: MassWalk (what the
// carried plane is and how it moves) and StepWalk (where eps, c1, c2 come from).  Nothing is selected at run time beyond
// diag_mass, full_refresh, draw_v0, noise and u, all wave-uniform.  `walk` takes the kernel's arguments BY VALUE: handed a
// reference to the kernel's parameter, the adapting massed kernels allocate 4 more VGPRs.
//
// Layout: rows.h -- a lane group is a chain; the structure is kinetic_kernel.h's (a persistent v plane, draw_v0, one store of x
// and v).  Transition: tempering_hmc_kernel.h's without the ladder, the LDS energy table and the barriers -- the trajectory is
// hmc::leapfrog_steps of hmc_kernel.h (the carried energy and force, the pseudo-transition t = -1, the merged kicks, the literal
// fallback), the kinetic energies are its helpers (IdentityKinetic, massed_kinetic), the Metropolis decision is spelled as
// hmc::metropolis_accept spells it, and the accept uniform as hmc_chain_body spells it.  What this walker adds: the partial refresh
// v = c1 v + c2 xi in front of the trajectory and one more slice, the post-refresh velocity, kept for the flip on a reject.  A
// chain never talks to another: no exchange, no atomic and no barrier beyond what Energy::eval needs; everything outside the
// chain's own registers (beta, the thinning test; the fixed eps, c1, c2; the adapting table row, delta, mu, the log bounds, the
// full-refresh test) is wave-uniform.
#pragma once
#include "chain_launch.h"
#include "hmc_kernel.h"
#include "landscape_energies.h"

namespace ebm {
namespace ghmc {
using namespace rows;

// ---- the argument structs: the fields every entry has, the two step-size parts, the two mass parts

struct WalkArgs {
  float* x;              // [n_chains, dim], in/out
  float* v;              // [n_chains, dim]: in/out, output only with draw_v0; under a mass the MOMENTUM plane p ~ N(0, T m)
  int64_t n_chains;
  int32_t dim, n_mh, n_leapfrog, thin, n_kept, draw_v0;
  float sqrt_temp, beta;  // fp32(sqrt T), fp32(1 / T)
  float* traj;           // [n_chains, n_kept, dim] or null
  uint8_t* accept_mask;  // [n_mh, n_chains] or null
  const float* noise;    // [n_mh, n_chains, dim] or null
  const float* u;        // [n_mh, n_chains] or null
  RngKey key;
  uint64_t step0;
  EnergyParams energy;
  int param_floats;
};

struct FixedStep {
  float eps, c1, c2;
};

struct AdaptStep {
  int32_t n_adapt, init_da, keep_open, full_refresh;  // init_da, keep_open: the two bits of the entry's init_da
  float eps0, gamma_l, temp;  // fp32(gamma L), fp32(T)
  float delta, mu, log_eps_min, log_eps_max;
  float* da;               // [3, n_chains]: eps, H-bar, log eps-bar; in/out, output only with init_da
  const float* da_table;   // [n_adapt, 5]: (1 - w, w, s, k, 1 - k)
  float* eps_trace;        // [n_mh, n_chains] or null
  float* alpha_mean;       // [n_chains] or null
};

struct UnitMass {};

struct Mass {
  int32_t mass_kind;     // EBM_MASS_SCALAR or EBM_MASS_DIAG
  float mass_raw, mass_sqrt, mass_safe;  // scalar mass forms
  const float* mass_diag;
};

template <class StepT, class MassT>
struct Args {
  WalkArgs w;
  StepT step;
  MassT mass;
};
using GhmcArgs = Args<FixedStep, UnitMass>;
using GhmcAdaptArgs = Args<AdaptStep, UnitMass>;
using GhmcAdaptMassArgs = Args<AdaptStep, Mass>;

namespace {

extern __shared__ __attribute__((aligned(16))) float ghmc_smem[];

// ---- the step-size axis: where eps, c1, c2 come from at the top of a transition, and what follows the decision

template <class StepT>
struct StepWalk;

// eps, c1, c2 are wave-uniform arguments
template <>
struct StepWalk<FixedStep> {
  const FixedStep s;
  template <class LaneT>
  __device__ __forceinline__ void load(const LaneT&, int64_t) {}
  __device__ __forceinline__ float eps() const { return s.eps; }
  __device__ __forceinline__ void refresh_constants(bool, float, float, float& c1, float& c2) const {
    c1 = s.c1;
    c2 = s.c2;
  }
  __device__ __forceinline__ void decided(int, float, float, bool, int64_t, int64_t) {}
  __device__ __forceinline__ void store(bool, int64_t, int64_t) const {}
};

// eps is a register of the chain (uniform within its lane group), the refresh constants c1, c2 follow it (two transcendental
// calls per transition when the friction is finite), and three floats of controller state -- eps, H-bar, log eps-bar -- ride
// beside the state from the one load to the one store
template <>
struct StepWalk<AdaptStep> {
  const AdaptStep s;
  float da0, hbar, lbar, alpha_sum;

  // the controller of this chain: every lane of the group holds the same three values (a lane without a chain: the start)
  template <class LaneT>
  __device__ __forceinline__ void load(const LaneT& L, int64_t n_chains) {
    da0 = s.eps0;
    hbar = 0.0f;
    lbar = 0.0f;
    if (!s.init_da && L.active) {  // (init_da: wave-uniform)
      da0 = s.da[L.chain];
      hbar = s.da[n_chains + L.chain];
      lbar = s.da[2 * n_chains + L.chain];
    }
    alpha_sum = 0.0f;
  }
  __device__ __forceinline__ float eps() const { return da0; }
  // the refresh constants at this chain's step size
  __device__ __forceinline__ void refresh_constants(bool init, float eps, float sqrt_temp, float& c1, float& c2) const {
    c1 = 0.0f;
    c2 = sqrt_temp;
    if (!s.full_refresh && !init) {  // wave-uniform
      const float span = s.gamma_l * eps;
      c1 = expf(-span);
      c2 = sqrtf(s.temp * (-expm1f(-2.0f * span)));
    }
  }
  __device__ __forceinline__ void decided(int t, float alpha, float eps, bool leader, int64_t chain, int64_t n_chains) {
    if (s.eps_trace && leader) s.eps_trace[(int64_t)t * n_chains + chain] = eps;
    // ---- dual averaging on this chain's own alpha (NaN counts as 0), every product and sum rounded on its own
    if (t < s.n_adapt) {  // wave-uniform
      const float* tab = s.da_table + 5 * t;  // wave-uniform row: (1 - w, w, s, k, 1 - k)
      const float al = (alpha == alpha) ? alpha : 0.0f;
      alpha_sum += al;
      hbar = tab[0] * hbar + tab[1] * (s.delta - al);
      float le = s.mu - tab[2] * hbar;
      le = le < s.log_eps_min ? s.log_eps_min : le;
      le = le > s.log_eps_max ? s.log_eps_max : le;
      lbar = tab[3] * le + tab[4] * lbar;
      da0 = expf((t + 1 == s.n_adapt && !s.keep_open) ? lbar : le);  // the close: the averaged iterate
    }
  }
  __device__ __forceinline__ void store(bool leader, int64_t chain, int64_t n_chains) const {
    if (leader) {
      s.da[chain] = da0;
      s.da[n_chains + chain] = hbar;
      s.da[2 * n_chains + chain] = lbar;
      if (s.alpha_mean) s.alpha_mean[chain] = s.n_adapt > 0 ? alpha_sum / (float)s.n_adapt : 0.0f;
    }
  }
};

// ---- the mass axis: the start scale of a drawn plane, the refresh coefficient per slot, the kinetic energy, the trajectory

template <class MassT, class LaneT>
struct MassWalk;

// the carried plane is the velocity v ~ N(0, T)
template <class LaneT>
struct MassWalk<UnitMass, LaneT> {
  const LaneT& L;
  const UnitMass m;
  __device__ __forceinline__ Slice<1> start(float sqrt_temp) {
    Slice<1> scale;
#pragma unroll
    for (int i = 0; i < 4; ++i) scale.a[0][i] = sqrt_temp;
    return scale;
  }
  __device__ __forceinline__ void set_step(float) {}
  __device__ __forceinline__ float refresh_coef(float c2, int) const { return c2; }
  __device__ __forceinline__ float kinetic(const Slice<1>& q) const { return hmc::IdentityKinetic<LaneT>{L}(q); }
  template <class En>
  __device__ __forceinline__ float trajectory(const En& en, Slice<1>& x, Slice<1>& p, Slice<1>& f, float eps_t, float half_eps,
                                              int n_lf, float e0, bool init) const {
    return hmc::leapfrog_steps<false>(en, L, x, p, f, x, eps_t, half_eps, n_lf, e0, init);
  }
};

// the carried plane is the MOMENTUM p ~ N(0, T m) under a step size per chain: the kinetic energy is hmc::massed_kinetic (the one
// hmc_chain_body calls) on m_raw, the trajectory hmc::leapfrog_steps<true> on drift = eps / m_safe, the refresh on c2 * m_sqrt --
// the per-slot forms of hmc::mass_forms.  The pseudo-transition t = -1 runs on the same drift: its momentum is zero, so
// x + drift * 0 is x as x + 0 * 0 is.
//
// Both products follow the chain's step size, so unlike ghmc_mass_kernel.h nothing of them can be formed in front of the loop:
// only m_raw lives through it, and m_sqrt, m_safe, the refresh coefficient and drift are re-formed from it at the top of every
// transition (the remedy docs/design/mass.md proposes under Cost).  The bits are those of forming them once: sqrtf is correctly
// rounded and m_safe is a compare.  The coefficient and m_sqrt die at the O step; across the trajectory the mass costs two slices
// (m_raw, drift) where ghmc_mass_kernel.h holds three.
template <class LaneT>
struct MassWalk<Mass, LaneT> {
  const LaneT& L;
  const Mass m;
  bool diag_mass;
  Slice<1> m_raw;  // the one mass form that lives through the loop
  Slice<1> m_now;  // m_raw behind the optimiser's back, of this transition
  Slice<1> drift;  // eps / max(m, 1e-10), of this transition

  __device__ __forceinline__ Slice<1> start(float sqrt_temp) {
    diag_mass = m.mass_kind == EBM_MASS_DIAG;
    Slice<1> m_sqrt, m_safe, scale;
    hmc::mass_forms(L, m, diag_mass, m_raw, m_sqrt, m_safe);
#pragma unroll
    for (int i = 0; i < 4; ++i) scale.a[0][i] = sqrt_temp * m_sqrt.a[0][i];
    return scale;
  }
  // drift = eps / m_safe at this chain's step size, re-formed from m_raw as hmc::mass_forms forms m_safe
  __device__ __forceinline__ void set_step(float eps) {
    m_now = m_raw;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      // (an empty statement the optimiser cannot see through: without it m_sqrt and m_safe are hoisted out of the loop as
      //  invariants and held across every trajectory, which is what re-forming them is there to avoid)
      asm volatile("" : "+v"(m_now.a[0][i]));
      const float m_safe = diag_mass ? (m_now.a[0][i] < 1e-10f ? 1e-10f : m_now.a[0][i]) : m.mass_safe;
      drift.a[0][i] = eps / m_safe;
    }
  }
  __device__ __forceinline__ float refresh_coef(float c2, int i) const {
    const float m_sqrt = diag_mass ? sqrtf(m_now.a[0][i]) : m.mass_sqrt;
    return c2 * m_sqrt;
  }
  __device__ __forceinline__ float kinetic(const Slice<1>& q) const {
    return hmc::massed_kinetic<true>(L, q, m_raw, diag_mass, m.mass_raw);
  }
  // the massed trajectory of hmc_chain_body at this chain's step size
  template <class En>
  __device__ __forceinline__ float trajectory(const En& en, Slice<1>& x, Slice<1>& p, Slice<1>& f, float eps_t, float half_eps,
                                              int n_lf, float e0, bool init) const {
    return hmc::leapfrog_steps<true>(en, L, x, p, f, drift, eps_t, half_eps, n_lf, e0, init);
  }
};

// ---- the walker

template <int KIND, int G, bool FULL, class StepT, class MassT>
__device__ __forceinline__ void walk(const Args<StepT, MassT> a) {
  using LaneT = Lane<G, 1, FULL>;
  const WalkArgs& w = a.w;
  LaneT L;
  L.init(w.n_chains, w.dim);
  const Smem S = carve_smem<1>(ghmc_smem, w.param_floats);
  stage_params(w.energy, w.dim, S.param);
  Energy<KIND, LaneT> en;
  en.init(w.energy, L, S);

  const int64_t row = L.active ? L.chain * (int64_t)w.dim : 0;
  const int64_t traj_row = L.active ? L.chain * (int64_t)w.n_kept * w.dim : 0;
  const float beta = w.beta;
  const bool leader = L.active && L.lg == 0;
  StepWalk<StepT> step{a.step};
  MassWalk<MassT, LaneT> mass{L, a.mass};
  Slice<1> xc, v;  // v: the carried velocity, or momentum
  load_slice(L, w.x, row, xc);
  {
    const Slice<1> scale = mass.start(w.sqrt_temp);
    if (w.draw_v0) {  // wave-uniform
      normal_slice(L, w.key, w.step0, v);
#pragma unroll
      for (int i = 0; i < 4; ++i) v.a[0][i] = L.ok(0, i) ? scale.a[0][i] * v.a[0][i] : 0.0f;
    } else {
      load_slice(L, w.v, row, v);
    }
  }
  step.load(L, w.n_chains);

  // energy and clamped force of the state the chain holds, carried from transition to transition; the pair of the initial
  // state comes out of the pseudo-transition t = -1 (hmc_kernel.h), which leaves v alone
  Slice<1> f;
#pragma unroll
  for (int i = 0; i < 4; ++i) f.a[0][i] = 0.0f;
  float e_cur = 0.0f;
  int kept = 0, until_keep = w.thin;

  for (int t = -1; t < w.n_mh; ++t) {
    const bool init = t < 0;
    const float eps = step.eps();
    const float eps_t = init ? 0.0f : eps;
    const float half_eps = 0.5f * eps_t;
    float c1, c2;
    step.refresh_constants(init, eps, w.sqrt_temp, c1, c2);
    mass.set_step(eps);

    // ---- O: the partial refresh, two products and a sum, each rounded on its own
    Slice<1> p;
    if (init) {
#pragma unroll
      for (int i = 0; i < 4; ++i) p.a[0][i] = 0.0f;
    } else {
      Slice<1> xi;
      if (w.noise) load_slice(L, w.noise, ((int64_t)t * w.n_chains) * w.dim + row, xi);
      else normal_slice(L, w.key, w.step0 + 1ull + 2ull * (uint64_t)t, xi);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float vo = c1 * v.a[0][i] + mass.refresh_coef(c2, i) * xi.a[0][i];
        p.a[0][i] = L.ok(0, i) ? vo : 0.0f;
      }
    }
    const Slice<1> v_o = p;  // the velocity after O: a reject hands back its negative

    // ---- the accept uniform of this chain, drawn in front of the trajectory as in hmc_chain_body
    float uu;
    if (init) uu = -1.0f;
    else if (w.u) uu = L.active ? w.u[(int64_t)t * w.n_chains + L.chain] : 2.0f;
    else uu = u01_half_open(pick(philox_at(w.key, (uint64_t)L.chain >> 2, w.step0 + 2ull + 2ull * (uint64_t)t),
                                 (int)(L.chain & 3)));

    // ---- H0 from the carried energy
    const float e0 = e_cur;
    const float h0 = clamp_nanprop(e0, -1e10f, 1e10f) + mass.kinetic(p);

    // ---- proposal
    const Slice<1> f_keep = f;
    Slice<1> x = xc;
    const int n_lf = init ? 1 : w.n_leapfrog;
    const float e1 = mass.trajectory(en, x, p, f, eps_t, half_eps, n_lf, e0, init);
    const float h1 = clamp_nanprop(e1, -1e10f, 1e10f) + mass.kinetic(p);

    // ---- Metropolis accept at the temperature T: the Hamiltonian of the target exp(-E / T) with v ~ N(0, T) -- p ~ N(0, T m)
    //      under a mass -- is beta (E + K).  Spelled as hmc::metropolis_accept spells it; alpha, the value the decision forms, is
    //      what an adapting step learns from
    const float dlt = clamp_nanprop(beta * (h0 - h1), -50.0f, 50.0f);
    float alpha = expf(dlt);
    alpha = (alpha > 1.0f) ? 1.0f : alpha;
    const bool accept = init || (L.active && (uu < alpha));
    if (accept) {
      e_cur = e1;
      xc = x;
    } else {
      f = f_keep;
    }
    if (init) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i) v.a[0][i] = accept ? p.a[0][i] : -v_o.a[0][i];  // the flip

    if (w.accept_mask && leader) w.accept_mask[(int64_t)t * w.n_chains + L.chain] = accept ? 1 : 0;
    step.decided(t, alpha, eps, leader, L.chain, w.n_chains);

    if (--until_keep == 0) {  // wave-uniform: (t + 1) % thin == 0
      until_keep = w.thin;
      if (w.traj && kept < w.n_kept) store_slice(L, w.traj, traj_row + (int64_t)kept * w.dim, xc);
      ++kept;
    }
  }
  store_slice(L, w.x, row, xc);
  store_slice(L, w.v, row, v);
  step.store(leader, L.chain, w.n_chains);
}

// ---- the three kernels, under the names profiles know them by

template <int KIND, int G, int NV, bool FULL>
__global__ __launch_bounds__(kBlock) void ghmc_chain(GhmcArgs a) {
  static_assert(NV == 1, "one vector per lane");
  walk<KIND, G, FULL>(a);
}

template <int KIND, int G, int NV, bool FULL>
__global__ __launch_bounds__(kBlock) void ghmc_adapt_chain(GhmcAdaptArgs a) {
  static_assert(NV == 1, "one vector per lane");
  walk<KIND, G, FULL>(a);
}

template <int KIND, int G, int NV, bool FULL>
__global__ __launch_bounds__(kBlock) void ghmc_adapt_mass_chain(GhmcAdaptMassArgs a) {
  static_assert(NV == 1, "one vector per lane");
  walk<KIND, G, FULL>(a);
}

}  // namespace

// The launchers of one energy kind: each is defined and instantiated in its family's unit (ghmc_unit.hip,
// ghmc_adapt_unit.hip, ghmc_adapt_mass_unit.hip; one object per family and kind).
template <int KIND>
void launch_kind(const Geometry& geo, dim3 grid, size_t smem, hipStream_t st, const GhmcArgs& a);
template <int KIND>
void launch_kind(const Geometry& geo, dim3 grid, size_t smem, hipStream_t st, const GhmcAdaptArgs& a);
template <int KIND>
void launch_kind(const Geometry& geo, dim3 grid, size_t smem, hipStream_t st, const GhmcAdaptMassArgs& a);

}  // namespace ghmc
}  // namespace ebm
