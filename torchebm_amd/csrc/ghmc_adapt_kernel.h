// Generalized HMC with per-chain dual-averaging step-size adaptation (Hoffman & Gelman 2014, section 3.2; Stan's shape: every
// chain adapts its own step size from its own acceptance probabilities): ebm_ghmc_adapt_chain_f32, include/ebm_hip_adapt.h;
// docs/design/adapt.md.
//
// The walker is ghmc_kernel.h's, statement for statement: rows.h lane groups, the persistent v plane, draw_v0, the
// pseudo-transition t = -1, hmc::leapfrog_steps<false>, IdentityKinetic, the flip, traj, accept_mask, the injected draws and the
// Philox coordinates.  What differs: eps is a register of the chain (uniform within its lane group) instead of a wave-uniform
// argument, the refresh constants c1, c2 follow it (two transcendental calls per transition when the friction is finite), and
// three floats of controller state -- eps, H-bar, log eps-bar -- ride beside the state from the one load to the one store.
// Nothing is reduced across chains: no exchange, no barrier beyond what Energy::eval needs, no atomic.  Everything outside the
// chain's own registers (the table row, delta, mu, the log bounds, beta, the full-refresh test, the thinning test) is wave-uniform.
#pragma once
#include "chain_launch.h"
#include "hmc_kernel.h"
#include "landscape_energies.h"

namespace ebm {
namespace ghmc_adapt {
using namespace rows;

struct GhmcAdaptArgs {
  float* x;              // [n_chains, dim], in/out
  float* v;              // [n_chains, dim]: in/out, output only with draw_v0
  int64_t n_chains;
  int32_t dim, n_mh, n_leapfrog, thin, n_kept, draw_v0;
  int32_t n_adapt, init_da, keep_open, full_refresh;  // init_da, keep_open: the two bits of the entry's init_da
  float eps0, gamma_l, temp, sqrt_temp, beta;  // fp32(gamma L), fp32(T), fp32(sqrt T), fp32(1 / T)
  float delta, mu, log_eps_min, log_eps_max;
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

extern __shared__ __attribute__((aligned(16))) float ghmc_adapt_smem[];

template <int KIND, int G, int NV, bool FULL>
__global__ __launch_bounds__(kBlock) void ghmc_adapt_chain(GhmcAdaptArgs a) {
  static_assert(NV == 1, "one vector per lane");
  using LaneT = Lane<G, 1, FULL>;
  LaneT L;
  L.init(a.n_chains, a.dim);
  const Smem S = carve_smem<1>(ghmc_adapt_smem, a.param_floats);
  stage_params(a.energy, a.dim, S.param);
  Energy<KIND, LaneT> en;
  en.init(a.energy, L, S);

  const int64_t row = L.active ? L.chain * (int64_t)a.dim : 0;
  const int64_t traj_row = L.active ? L.chain * (int64_t)a.n_kept * a.dim : 0;
  const float beta = a.beta;
  const bool leader = L.active && L.lg == 0;
  Slice<1> xc, v;
  load_slice(L, a.x, row, xc);
  if (a.draw_v0) {  // wave-uniform
    normal_slice(L, a.key, a.step0, v);
#pragma unroll
    for (int i = 0; i < 4; ++i) v.a[0][i] = L.ok(0, i) ? a.sqrt_temp * v.a[0][i] : 0.0f;
  } else {
    load_slice(L, a.v, row, v);
  }

  // the controller of this chain: every lane of the group holds the same three values (a lane without a chain: the start)
  float da0 = a.eps0, hbar = 0.0f, lbar = 0.0f;
  if (!a.init_da && L.active) {  // (init_da: wave-uniform)
    da0 = a.da[L.chain];
    hbar = a.da[a.n_chains + L.chain];
    lbar = a.da[2 * a.n_chains + L.chain];
  }
  float alpha_sum = 0.0f;

  const hmc::IdentityKinetic<LaneT> kinetic{L};

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

    // ---- the accept uniform of this chain, drawn in front of the trajectory as in hmc_chain_body
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
    for (int i = 0; i < 4; ++i) v.a[0][i] = accept ? p.a[0][i] : -v_o.a[0][i];  // the flip

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

// The launcher of one energy kind: defined and instantiated in ghmc_adapt_unit.hip (one object per kind).
template <int KIND>
void launch_kind(const Geometry& geo, dim3 grid, size_t smem, hipStream_t st, const GhmcAdaptArgs& a);

}  // namespace ghmc_adapt
}  // namespace ebm
