// Kernel body of underdamped Langevin, BAOAB, with a scalar or diagonal mass on the wide MLP energy
// (ebm_kinetic_mlp_chain_mass_f32, include/ebm_hip_mass_mlp.h; docs/design/mass_mlp.md): the walk of mlp_wide_kinetic_body.h whose carried
// plane is the MOMENTUM p ~ N(0, T m).  The one-evaluation-site loop, the unmerged kicks p - hh g, rows, noise and Philox
// coordinates are the unit-mass walk's; the two drifts run on a_j = hh / m_safe_j and the O step on s_j = c2 m_sqrt_j, formed once
// per workgroup into LDS tables (mlp_wide_mass.h) and read a register quad at a time inside the step, so no mass form lives in
// registers through an evaluation.  With every factor 1 the kernel computes the unit-mass walk's bits.  Two translation units
// instantiate it: mlp_wide_kinetic_mass.hip (H = 64) and mlp_wide_kinetic_mass_h128.hip (H = 128).
#pragma once
#include "mlp_wide_mass.h"

namespace ebm {
namespace widemlp {

struct WideKineticMassArgs {
  float* x;             // [n_chains, dim], in/out
  float* v;             // [n_chains, dim], the momentum plane: in/out, output only with draw_v0
  int64_t n_chains;
  int32_t dim, k_steps, thin, n_kept, draw_v0;
  float hh, c1, c2, sqrt_temp;
  int32_t mass_kind;    // EBM_MASS_SCALAR or EBM_MASS_DIAG
  float mass_raw, mass_sqrt, mass_safe;  // scalar mass forms
  const float* mass_diag;                // [dim] or null
  float* traj;          // [n_chains, n_kept, dim] or null
  const float* noise;   // [k_steps, n_chains, dim] or null
  RngKey key;
  uint64_t step0;
  const float* params;
  const char* w1_image;  // always null: the shared set-up text names it for MODE 3, which this kernel is not built for
};

constexpr int kKineticMassTables = 3;  // a = hh / m_safe, s = c2 m_sqrt, m_sqrt (the start draw's)

template <int HT, int DT, int MODE>
__global__ __launch_bounds__(kBlock, 1) void mlp_wide_kinetic_mass_chain(WideKineticMassArgs a) {
  static_assert(MODE == 0 || MODE == 2, "weights in LDS: fp32 (0) or split bf16 images (2)");
  constexpr bool EVAL_SCALED = false;
#include "mlp_wide_setup.inc"
  EBM_WIDE_WALKS_ONCE_OPAQUE();  // (mlp_wide_rows.h)
  EBM_WIDE_LANES();

  // the tables, behind the unit-mass layout: 1 at and beyond dim
  float* const drift_tab = wide_smem + wide_smem_bytes(HT, DT, MODE) / sizeof(float);
  float* const refresh_tab = drift_tab + kMassCols;
  float* const sqrt_tab = refresh_tab + kMassCols;
  for (int c = threadIdx.x; c < kMassCols; c += kBlock) {
    float m_raw, m_sqrt, m_safe;
    mass_forms_at(a, c, m_raw, m_sqrt, m_safe);
    drift_tab[c] = c < dim ? a.hh / m_safe : 1.0f;
    refresh_tab[c] = c < dim ? a.c2 * m_sqrt : 1.0f;
    sqrt_tab[c] = m_sqrt;
  }
  __syncthreads();

  const float hh = a.hh, c1 = a.c1;
  float xr[DT][16], p[DT][16];
  load_rows(lanes, xr, a.x, sample);
  if (a.draw_v0) {  // wave-uniform: p = (sqrt_temp m_sqrt) z0, the field at step0 -- the unit-mass walk's block with the table's
                    // factor, spelled here: as a helper that takes the argument struct it cost every kernel above DT = 1 between 26
                    // and 92 AGPRs and the two DT = 4 kernels 368 / 524 bytes of scratch (docs/design/mass_mlp.md)
#pragma unroll
    for (int td = 0; td < DT; ++td)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float z[4], ms[4];
        normal_quad(lanes, z, a.key, 32 * td + 8 * q + 4 * h, sample, a.step0);
        table_quad(ms, sqrt_tab, 32 * td + 8 * q + 4 * h);
#pragma unroll
        for (int i = 0; i < 4; ++i) p[td][4 * q + i] = (32 * td + 8 * q + 4 * h + i < dim) ? (a.sqrt_temp * ms[i]) * z[i] : 0.0f;
      }
  } else {
    load_rows(lanes, p, a.v, sample);
  }

  int kept = 0, until_keep = a.thin;
  for (int i = 0;; ++i) {  // wave-uniform
    EBM_WIDE_STEP_COPIES_OPAQUE();  // smp, hq, key (mlp_wide_rows.h)
    constexpr bool eval_need_energy = false;
#include "mlp_wide_plain_eval.inc"
    // (the energy's chain is kept alive by a use that issues nothing: mlp_wide_kinetic_body.h says why)
    asm volatile("" ::"v"(energy));
    if (i > 0) {   // the closing B of step i - 1
#pragma unroll
      for (int td = 0; td < DT; ++td)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float pi = p[td][r] - hh * g[td][r];
          p[td][r] = (32 * td + row_of(r, hq) < dim) ? pi : 0.0f;
        }
      if (--until_keep == 0) {  // i % thin == 0
        until_keep = a.thin;
        if (a.traj && kept < a.n_kept && active) store_rows(lanes, a.traj, smp * (int64_t)a.n_kept + kept, xr);
        ++kept;
      }
    }
    if (i == a.k_steps) break;
    // step i: B, A, O, A -- every operation rounded on its own, a register quad at a time; the quad's a and s come from LDS
    // here (hq is this iteration's opaque copy: nothing of a table is carried round the loop)
    const float* noise_i = a.noise ? a.noise + (int64_t)i * a.n_chains * dim : nullptr;
#pragma unroll
    for (int td = 0; td < DT; ++td)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c0 = 32 * td + 8 * q + 4 * hq;
        EBM_WIDE_NOISE_QUAD(z, noise_i, lanes, a.step0 + 1ull + (uint64_t)i);  // (mlp_wide_rows.h)
        float am[4], sm[4];
        table_quad(am, drift_tab, c0);
        table_quad(sm, refresh_tab, c0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int r = 4 * q + j;
          float pi = p[td][r] - hh * g[td][r];
          float xv = xr[td][r] + am[j] * pi;
          pi = c1 * pi + sm[j] * z[j];
          xv = xv + am[j] * pi;
          xr[td][r] = (c0 + j < dim) ? xv : 0.0f;
          p[td][r] = (c0 + j < dim) ? pi : 0.0f;
        }
      }
  }
  if (active) {
    store_rows(lanes, a.x, sample, xr);
    store_rows(lanes, a.v, sample, p);
  }
}

struct KineticMassWalk {  // (launch_massed_walk_by_dim, mlp_wide_mass.h)
  template <int HT, int DT, int MODE>
  static constexpr auto kernel = &mlp_wide_kinetic_mass_chain<HT, DT, MODE>;
  static constexpr int tables = kKineticMassTables;
};

}  // namespace widemlp
}  // namespace ebm
