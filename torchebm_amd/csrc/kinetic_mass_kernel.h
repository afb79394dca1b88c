// Underdamped Langevin, BAOAB, with a scalar or diagonal mass: the walker of kinetic_kernel.h whose carried plane is the
// MOMENTUM p ~ N(0, T m) (ebm_kinetic_chain_mass_f32, include/ebm_hip.h; docs/design/mass.md).
//
// Layout: kinetic_kernel.h's -- a lane group is a chain; x, p and g are one slice each.  The mass adds two slices that live
// through the loop, a = hh / m_safe and s = c2 * m_sqrt, formed once in front of it from the three per-slot forms of
// hmc_kernel.h (mass_forms: the block hmc_chain_body runs); the forms themselves die there, m_sqrt after the start draw.
// With every m = 1 each line below is kinetic_kernel.h's with an exact factor (hh / 1, c2 * 1), so the bits are its bits.
#pragma once
#include "chain_launch.h"
#include "hmc_kernel.h"
#include "landscape_energies.h"

namespace ebm {
namespace kinetic_mass {
using namespace rows;

struct KineticMassArgs {
  float* x;            // [n_chains, dim], in/out
  float* v;            // [n_chains, dim], the momentum plane: in/out, output only with draw_v0
  int64_t n_chains;
  int32_t dim, k_steps, thin, n_kept, draw_v0;
  float hh, c1, c2, sqrt_temp;
  int32_t mass_kind;   // EBM_MASS_SCALAR or EBM_MASS_DIAG
  float mass_raw, mass_sqrt, mass_safe;  // scalar mass forms
  const float* mass_diag;
  float* traj;         // [n_chains, n_kept, dim] or null
  const float* noise;  // [k_steps, n_chains, dim] or null
  RngKey key;
  uint64_t step0;
  EnergyParams energy;
  int param_floats;
};

namespace {

extern __shared__ __attribute__((aligned(16))) float kinetic_mass_smem[];

template <int KIND, int G, int NV, bool FULL>
__global__ __launch_bounds__(kBlock) void kinetic_mass_chain(KineticMassArgs a) {
  static_assert(NV == 1, "one vector per lane");
  using LaneT = Lane<G, 1, FULL>;
  LaneT L;
  L.init(a.n_chains, a.dim);
  const Smem S = carve_smem<1>(kinetic_mass_smem, a.param_floats);
  stage_params(a.energy, a.dim, S.param);
  Energy<KIND, LaneT> en;
  en.init(a.energy, L, S);

  const int64_t row = L.active ? L.chain * (int64_t)a.dim : 0;
  const int64_t traj_row = L.active ? L.chain * (int64_t)a.n_kept * a.dim : 0;
  const float hh = a.hh, c1 = a.c1;
  Slice<1> x, p, g;
  load_slice(L, a.x, row, x);

  // a = hh / max(m, 1e-10) and s = c2 * sqrt(m) per slot, and the start scale sqrt_temp * sqrt(m)
  Slice<1> drift, kick;
  {
    Slice<1> m_raw, m_sqrt, m_safe;
    hmc::mass_forms(L, a, a.mass_kind == EBM_MASS_DIAG, m_raw, m_sqrt, m_safe);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      drift.a[0][i] = hh / m_safe.a[0][i];
      kick.a[0][i] = a.c2 * m_sqrt.a[0][i];
    }
    if (a.draw_v0) {  // wave-uniform
      normal_slice(L, a.key, a.step0, p);
#pragma unroll
      for (int i = 0; i < 4; ++i) p.a[0][i] = L.ok(0, i) ? (a.sqrt_temp * m_sqrt.a[0][i]) * p.a[0][i] : 0.0f;
    } else {
      load_slice(L, a.v, row, p);
    }
  }
  en.template eval<false>(L, x, g);  // the raw gradient, no clamp: a NaN stays in its chain

  int kept = 0, until_keep = a.thin;
  for (int s = 0; s < a.k_steps; ++s) {
    Slice<1> xi;
    if (a.noise) load_slice(L, a.noise, ((int64_t)s * a.n_chains) * a.dim + row, xi);
    else normal_slice(L, a.key, a.step0 + 1ull + (uint64_t)s, xi);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      // B, A, O, A: every operation rounded on its own
      float pi = p.a[0][i] - hh * g.a[0][i];
      float xv = x.a[0][i] + drift.a[0][i] * pi;
      pi = c1 * pi + kick.a[0][i] * xi.a[0][i];
      xv = xv + drift.a[0][i] * pi;
      x.a[0][i] = L.ok(0, i) ? xv : 0.0f;
      p.a[0][i] = L.ok(0, i) ? pi : 0.0f;
    }
    en.template eval<false>(L, x, g);
#pragma unroll
    for (int i = 0; i < 4; ++i) {  // B
      const float pi = p.a[0][i] - hh * g.a[0][i];
      p.a[0][i] = L.ok(0, i) ? pi : 0.0f;
    }
    if (--until_keep == 0) {  // wave-uniform: (s + 1) % thin == 0
      until_keep = a.thin;
      if (a.traj && kept < a.n_kept) store_slice(L, a.traj, traj_row + (int64_t)kept * a.dim, x);
      ++kept;
    }
  }
  store_slice(L, a.x, row, x);
  store_slice(L, a.v, row, p);
}

}  // namespace

// The launcher of one energy kind: defined and instantiated in kinetic_mass_unit.hip (one object per kind).
template <int KIND>
void launch_kind(const Geometry& geo, dim3 grid, size_t smem, hipStream_t st, const KineticMassArgs& a);

}  // namespace kinetic_mass
}  // namespace ebm
