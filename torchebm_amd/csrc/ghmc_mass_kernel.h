// Generalized HMC with a scalar or diagonal mass: the walker of ghmc_kernel.h whose carried plane is the MOMENTUM
// p ~ N(0, T m) (ebm_ghmc_chain_mass_f32, include/ebm_hip.h; docs/design/mass.md).
//
// Layout and transition: ghmc_kernel.h's.  The mass adds three slices that live through the loop: m_raw for the kinetic
// energy (hmc::massed_kinetic, the one hmc_chain_body calls), drift = eps / m_safe for hmc::leapfrog_steps<true>, and
// s = c2 * m_sqrt for the refresh -- formed once in front of the loop from the per-slot forms of hmc::mass_forms.  The
// pseudo-transition t = -1 runs on the same drift: its momentum is zero, so x + drift * 0 is x as x + 0 * 0 is.
#pragma once
#include "chain_launch.h"
#include "hmc_kernel.h"
#include "landscape_energies.h"

namespace ebm {
namespace ghmc_mass {
using namespace rows;

struct GhmcMassArgs {
  float* x;              // [n_chains, dim], in/out
  float* v;              // [n_chains, dim], the momentum plane: in/out, output only with draw_v0
  int64_t n_chains;
  int32_t dim, n_mh, n_leapfrog, thin, n_kept, draw_v0;
  float eps, c1, c2, sqrt_temp, beta;
  int32_t mass_kind;     // EBM_MASS_SCALAR or EBM_MASS_DIAG
  float mass_raw, mass_sqrt, mass_safe;  // scalar mass forms
  const float* mass_diag;
  float* traj;           // [n_chains, n_kept, dim] or null
  uint8_t* accept_mask;  // [n_mh, n_chains] or null
  const float* noise;    // [n_mh, n_chains, dim] or null
  const float* u;        // [n_mh, n_chains] or null
  RngKey key;
  uint64_t step0;
  EnergyParams energy;
  int param_floats;
};

namespace {

extern __shared__ __attribute__((aligned(16))) float ghmc_mass_smem[];

template <int KIND, int G, int NV, bool FULL>
__global__ __launch_bounds__(kBlock) void ghmc_mass_chain(GhmcMassArgs a) {
  static_assert(NV == 1, "one vector per lane");
  using LaneT = Lane<G, 1, FULL>;
  LaneT L;
  L.init(a.n_chains, a.dim);
  const Smem S = carve_smem<1>(ghmc_mass_smem, a.param_floats);
  stage_params(a.energy, a.dim, S.param);
  Energy<KIND, LaneT> en;
  en.init(a.energy, L, S);

  const int64_t row = L.active ? L.chain * (int64_t)a.dim : 0;
  const int64_t traj_row = L.active ? L.chain * (int64_t)a.n_kept * a.dim : 0;
  const float c1 = a.c1, beta = a.beta;
  const bool leader = L.active && L.lg == 0;
  const bool diag_mass = a.mass_kind == EBM_MASS_DIAG;
  Slice<1> xc, v;  // v: the carried momentum
  load_slice(L, a.x, row, xc);

  Slice<1> m_raw, drift, refresh;  // m, eps / max(m, 1e-10), c2 * sqrt(m)
  {
    Slice<1> m_sqrt, m_safe;
    hmc::mass_forms(L, a, diag_mass, m_raw, m_sqrt, m_safe);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      drift.a[0][i] = a.eps / m_safe.a[0][i];
      refresh.a[0][i] = a.c2 * m_sqrt.a[0][i];
    }
    if (a.draw_v0) {  // wave-uniform
      normal_slice(L, a.key, a.step0, v);
#pragma unroll
      for (int i = 0; i < 4; ++i) v.a[0][i] = L.ok(0, i) ? (a.sqrt_temp * m_sqrt.a[0][i]) * v.a[0][i] : 0.0f;
    } else {
      load_slice(L, a.v, row, v);
    }
  }

  auto kinetic = [&](const Slice<1>& q) -> float { return hmc::massed_kinetic<true>(L, q, m_raw, diag_mass, a.mass_raw); };

  // energy and clamped force of the state the chain holds, carried from transition to transition; the pair of the initial
  // state comes out of the pseudo-transition t = -1 (hmc_kernel.h), which leaves the momentum alone
  Slice<1> f;
#pragma unroll
  for (int i = 0; i < 4; ++i) f.a[0][i] = 0.0f;
  float e_cur = 0.0f;
  int kept = 0, until_keep = a.thin;

  for (int t = -1; t < a.n_mh; ++t) {
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
        const float po = c1 * v.a[0][i] + refresh.a[0][i] * xi.a[0][i];
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

    // ---- proposal: the massed trajectory of hmc_chain_body, the drift one FMA with eps / m
    const Slice<1> f_keep = f;
    Slice<1> x = xc;
    const int n_lf = init ? 1 : a.n_leapfrog;
    const float e1 = hmc::leapfrog_steps<true>(en, L, x, p, f, drift, eps_t, half_eps, n_lf, e0, init);
    const float h1 = clamp_nanprop(e1, -1e10f, 1e10f) + kinetic(p);

    // ---- Metropolis accept at the temperature T: the Hamiltonian of exp(-E / T) with p ~ N(0, T m) is beta (E + K_m(p))
    const bool accept = hmc::metropolis_accept(beta * (h0 - h1), uu, init, L.active);
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

    if (--until_keep == 0) {  // wave-uniform: (t + 1) % thin == 0
      until_keep = a.thin;
      if (a.traj && kept < a.n_kept) store_slice(L, a.traj, traj_row + (int64_t)kept * a.dim, xc);
      ++kept;
    }
  }
  store_slice(L, a.x, row, xc);
  store_slice(L, a.v, row, v);
}

}  // namespace

// The launcher of one energy kind: defined and instantiated in ghmc_mass_unit.hip (one object per kind).
template <int KIND>
void launch_kind(const Geometry& geo, dim3 grid, size_t smem, hipStream_t st, const GhmcMassArgs& a);

}  // namespace ghmc_mass
}  // namespace ebm
