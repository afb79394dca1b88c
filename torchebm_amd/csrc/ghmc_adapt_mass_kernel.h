// Generalized HMC with a scalar or diagonal mass AND per-chain dual-averaging step-size adaptation:
// ebm_ghmc_adapt_chain_mass_f32, include/ebm_hip_adapt_mass.h; docs/design/adapt_mass.md.
//
// The walker is ghmc_adapt_kernel.h's, statement for statement -- eps a register of the chain, the refresh constants following
// it, three floats of controller state beside the state -- with ghmc_mass_kernel.h's mass: the carried plane is the MOMENTUM
// p ~ N(0, T m), the kinetic energy hmc::massed_kinetic, the trajectory hmc::leapfrog_steps<true> on drift = eps / m_safe, the
// refresh on c2 * m_sqrt.  Both products follow the chain's step size, so unlike ghmc_mass_kernel.h nothing of them can be
// formed in front of the loop: only m_raw lives through it, and m_sqrt, m_safe, refresh and drift are re-formed from it at the
// top of every transition (the remedy docs/design/mass.md proposes under Cost).  The bits are those of forming them once:
// sqrtf is correctly rounded and m_safe is a compare.  refresh and m_sqrt die at the O step; across the trajectory the mass
// costs two slices (m_raw, drift) where ghmc_mass_kernel.h holds three.
#pragma once
#include "chain_launch.h"
#include "hmc_kernel.h"
#include "landscape_energies.h"

namespace ebm {
namespace ghmc_adapt_mass {
using namespace rows;

struct GhmcAdaptMassArgs {
  float* x;              // [n_chains, dim], in/out
  float* v;              // [n_chains, dim], the momentum plane: in/out, output only with draw_v0
  int64_t n_chains;
  int32_t dim, n_mh, n_leapfrog, thin, n_kept, draw_v0;
  int32_t n_adapt, init_da, keep_open, full_refresh;  // init_da, keep_open: the two bits of the entry's init_da
  float eps0, gamma_l, temp, sqrt_temp, beta;  // fp32(gamma L), fp32(T), fp32(sqrt T), fp32(1 / T)
  float delta, mu, log_eps_min, log_eps_max;
  int32_t mass_kind;     // EBM_MASS_SCALAR or EBM_MASS_DIAG
  float mass_raw, mass_sqrt, mass_safe;  // scalar mass forms
  const float* mass_diag;
  float* da;               // [3, n_chains]: eps, H-bar, log eps-bar; in/out, output only with init_da
  const float* da_table;   // [n_adapt, 5]: (1 - w, w, s, k, 1 - k)
  float* eps_trace;        // [n_mh, n_chains] or null
  float* alpha_mean;       // [n_chains] or null
  float* traj;             // [n_chains, n_kept, dim] or null
  uint8_t* accept_mask;    // [n_mh, n_chains] or null
  const float* noise;      // [n_mh, n_chains, dim] or null
  const float* u;          // [n_mh, n_chains] or null
  RngKey key;
  uint64_t step0;
  EnergyParams energy;
  int param_floats;
};

namespace {

extern __shared__ __attribute__((aligned(16))) float ghmc_adapt_mass_smem[];

template <int KIND, int G, int NV, bool FULL>
__global__ __launch_bounds__(kBlock) void ghmc_adapt_mass_chain(GhmcAdaptMassArgs a) {
  static_assert(NV == 1, "one vector per lane");
  using LaneT = Lane<G, 1, FULL>;
  LaneT L;
  L.init(a.n_chains, a.dim);
  const Smem S = carve_smem<1>(ghmc_adapt_mass_smem, a.param_floats);
  stage_params(a.energy, a.dim, S.param);
  Energy<KIND, LaneT> en;
  en.init(a.energy, L, S);

  const int64_t row = L.active ? L.chain * (int64_t)a.dim : 0;
  const int64_t traj_row = L.active ? L.chain * (int64_t)a.n_kept * a.dim : 0;
  const float beta = a.beta;
  const bool leader = L.active && L.lg == 0;
  const bool diag_mass = a.mass_kind == EBM_MASS_DIAG;
  Slice<1> xc, v;  // v: the carried momentum
  load_slice(L, a.x, row, xc);

  Slice<1> m_raw;  // the one mass form that lives through the loop
  {
    Slice<1> m_sqrt, m_safe;
    hmc::mass_forms(L, a, diag_mass, m_raw, m_sqrt, m_safe);
    if (a.draw_v0) {  // wave-uniform
      normal_slice(L, a.key, a.step0, v);
#pragma unroll
      for (int i = 0; i < 4; ++i) v.a[0][i] = L.ok(0, i) ? (a.sqrt_temp * m_sqrt.a[0][i]) * v.a[0][i] : 0.0f;
    } else {
      load_slice(L, a.v, row, v);
    }
  }

  // the controller of this chain: every lane of the group holds the same three values (a lane without a chain: the start)
  float da0 = a.eps0, hbar = 0.0f, lbar = 0.0f;
  if (!a.init_da && L.active) {  // (init_da: wave-uniform)
    da0 = a.da[L.chain];
    hbar = a.da[a.n_chains + L.chain];
    lbar = a.da[2 * a.n_chains + L.chain];
  }
  float alpha_sum = 0.0f;

  auto kinetic = [&](const Slice<1>& q) -> float { return hmc::massed_kinetic<true>(L, q, m_raw, diag_mass, a.mass_raw); };

  // energy and clamped force of the state the chain holds, carried from transition to transition (ghmc_kernel.h)
  Slice<1> f;
#pragma unroll
  for (int i = 0; i < 4; ++i) f.a[0][i] = 0.0f;
  float e_cur = 0.0f;
  int kept = 0, until_keep = a.thin;

  for (int t = -1; t < a.n_mh; ++t) {
    const bool init = t < 0;
    const float eps = da0;
    const float eps_t = init ? 0.0f : eps;
    const float half_eps = 0.5f * eps_t;

    // ---- the refresh constants at this chain's step size
    float c1 = 0.0f, c2 = a.sqrt_temp;
    if (!a.full_refresh && !init) {  // wave-uniform
      const float span = a.gamma_l * eps;
      c1 = expf(-span);
      c2 = sqrtf(a.temp * (-expm1f(-2.0f * span)));
    }

    // ---- drift = eps / m_safe, re-formed from m_raw as hmc::mass_forms forms m_safe (the pseudo-transition runs on the same
    //      drift: its momentum is zero, as in ghmc_mass_kernel.h)
    Slice<1> drift, m_now = m_raw;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      // (an empty statement the optimiser cannot see through: without it m_sqrt and m_safe are hoisted out of the loop as
      //  invariants and held across every trajectory, which is what re-forming them is there to avoid)
      asm volatile("" : "+v"(m_now.a[0][i]));
      const float m_safe = diag_mass ? (m_now.a[0][i] < 1e-10f ? 1e-10f : m_now.a[0][i]) : a.mass_safe;
      drift.a[0][i] = eps / m_safe;
    }

    // ---- O: the partial refresh on refresh = c2 * m_sqrt, two products and a sum, each rounded on its own
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
        const float m_sqrt = diag_mass ? sqrtf(m_now.a[0][i]) : a.mass_sqrt;
        const float refresh = c2 * m_sqrt;
        const float po = c1 * v.a[0][i] + refresh * xi.a[0][i];
        p.a[0][i] = L.ok(0, i) ? po : 0.0f;
      }
    }
    const Slice<1> p_o = p;  // the momentum after O: a reject hands back its negative

    // ---- the accept uniform of this chain, drawn in front of the trajectory as in hmc_chain_body
    float uu;
    if (init) uu = -1.0f;
    else if (a.u) uu = L.active ? a.u[(int64_t)t * a.n_chains + L.chain] : 2.0f;
    else uu = u01_half_open(pick(philox_at(a.key, (uint64_t)L.chain >> 2, a.step0 + 2ull + 2ull * (uint64_t)t),
                                 (int)(L.chain & 3)));

    // ---- H0 from the carried energy
    const float e0 = e_cur;
    const float h0 = clamp_nanprop(e0, -1e10f, 1e10f) + kinetic(p);

    // ---- proposal: the massed trajectory of hmc_chain_body at this chain's step size
    const Slice<1> f_keep = f;
    Slice<1> x = xc;
    const int n_lf = init ? 1 : a.n_leapfrog;
    const float e1 = hmc::leapfrog_steps<true>(en, L, x, p, f, drift, eps_t, half_eps, n_lf, e0, init);
    const float h1 = clamp_nanprop(e1, -1e10f, 1e10f) + kinetic(p);

    // ---- Metropolis accept, spelled as hmc::metropolis_accept spells it; alpha is the value the decision forms
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
    for (int i = 0; i < 4; ++i) v.a[0][i] = accept ? p.a[0][i] : -p_o.a[0][i];  // the flip

    if (a.accept_mask && leader) a.accept_mask[(int64_t)t * a.n_chains + L.chain] = accept ? 1 : 0;
    if (a.eps_trace && leader) a.eps_trace[(int64_t)t * a.n_chains + L.chain] = eps;

    // ---- dual averaging on this chain's own alpha (NaN counts as 0), every product and sum rounded on its own
    if (t < a.n_adapt) {  // wave-uniform
      const float* tab = a.da_table + 5 * t;  // wave-uniform row: (1 - w, w, s, k, 1 - k)
      const float al = (alpha == alpha) ? alpha : 0.0f;
      alpha_sum += al;
      hbar = tab[0] * hbar + tab[1] * (a.delta - al);
      float le = a.mu - tab[2] * hbar;
      le = le < a.log_eps_min ? a.log_eps_min : le;
      le = le > a.log_eps_max ? a.log_eps_max : le;
      lbar = tab[3] * le + tab[4] * lbar;
      da0 = expf((t + 1 == a.n_adapt && !a.keep_open) ? lbar : le);  // the close: the averaged iterate
    }

    if (--until_keep == 0) {  // wave-uniform: (t + 1) % thin == 0
      until_keep = a.thin;
      if (a.traj && kept < a.n_kept) store_slice(L, a.traj, traj_row + (int64_t)kept * a.dim, xc);
      ++kept;
    }
  }
  store_slice(L, a.x, row, xc);
  store_slice(L, a.v, row, v);
  if (leader) {
    a.da[L.chain] = da0;
    a.da[a.n_chains + L.chain] = hbar;
    a.da[2 * a.n_chains + L.chain] = lbar;
    if (a.alpha_mean) a.alpha_mean[L.chain] = a.n_adapt > 0 ? alpha_sum / (float)a.n_adapt : 0.0f;
  }
}

}  // namespace

// The launcher of one energy kind: defined and instantiated in ghmc_adapt_mass_unit.hip (one object per kind).
template <int KIND>
void launch_kind(const Geometry& geo, dim3 grid, size_t smem, hipStream_t st, const GhmcAdaptMassArgs& a);

}  // namespace ghmc_adapt_mass
}  // namespace ebm
