// Kernel body of the running moments of underdamped Langevin dynamics, BAOAB, on the wide MLP energy (sampler 0 of
// ebm_kinetic_moments_mlp_f32, include/ebm_hip.h; docs/design/kinetic_moments_mlp.md): the walk of mlp_wide_kinetic_body.h,
// operation for operation -- ONE evaluation site, k_steps + 1 evaluations, the two kicks never merged, the raw gradient, z_i at
// Philox step step0 + 1 + i -- with the Welford pairs of ebm_kinetic_moments_f32 beside it.  Two translation units instantiate it
// (compiled in parallel): mlp_wide_kinetic_moments.hip (H = 64) and mlp_wide_kinetic_moments_h128.hip (H = 128).
//
// Where the pairs live.  Not in registers: the plain kernel holds 256 VGPRs, and two more planes of 16 DT registers through
// every evaluation do not fit.  They live in the caller's mom / e_mom / v2_mom planes and are updated in place once per counted
// step (moments_rows, mlp_wide_rows.h), where the plain body keeps its trajectory: behind the closing B, when the gradient and
// everything of the evaluation is dead.  A lane reads back only what it stored itself, through an opaque copy of the pointer (as
// the flip of mlp_wide_ghmc_body.h does); at c == 1 the planes are not read.  The half switch is a wave-uniform plane offset.
//
// The energy of a counted state costs nothing: evaluation i >= 1 is made at the position behind step i - 1, which is the
// counted state, and its energy chain is alive in the plain kernel already.
#pragma once
#include "mlp_wide_rows.h"

namespace ebm {
namespace widemlp {

struct WideKineticMomentsArgs {
  float* x;             // [n_chains, dim], in/out
  float* v;             // [n_chains, dim]: in/out, output only with draw_v0
  int64_t n_chains;
  int32_t dim, k_steps, burn_in, half_len, draw_v0;
  float hh, c1, c2, sqrt_temp;
  const float* recip;   // device [half_len]: float32(1 / c), c = 1 .. half_len
  float* mom;           // [4, n_chains, dim]: mean_a, M2_a, mean_b, M2_b -- working storage during the launch
  float* e_mom;         // [4, n_chains] or null
  float* v2_mom;        // [2, n_chains, dim] or null: the mean of v^2 of either half
  float* traj;          // [n_chains, 2 half_len, dim] or null
  float* e_traj;        // [n_chains, 2 half_len] or null
  float* v_traj;        // [n_chains, 2 half_len, dim] or null
  const float* noise;   // [k_steps, n_chains, dim] or null
  RngKey key;
  uint64_t step0;
  const float* params;
  const char* w1_image;  // always null: the shared set-up text names it for MODE 3, which this kernel is not built for
};

template <int HT, int DT, int MODE>
__global__ __launch_bounds__(kBlock, 1) void mlp_wide_kinetic_moments_chain(WideKineticMomentsArgs a) {
  static_assert(MODE == 0 || MODE == 2, "weights in LDS: fp32 (0) or split bf16 images (2)");
  constexpr bool EVAL_SCALED = false;
#include "mlp_wide_setup.inc"
  EBM_WIDE_WALKS_ONCE_OPAQUE();  // (mlp_wide_rows.h)
  EBM_WIDE_LANES();

  const float hh = a.hh, c1 = a.c1, c2 = a.c2;
  float xr[DT][16], v[DT][16];
  load_rows(lanes, xr, a.x, sample);
  if (a.draw_v0) {  // wave-uniform: v = sqrt_temp z0, the field at step0
#pragma unroll
    for (int td = 0; td < DT; ++td)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float z[4];
        normal_quad(lanes, z, a.key, 32 * td + 8 * q + 4 * h, sample, a.step0);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[td][4 * q + i] = (32 * td + 8 * q + 4 * h + i < dim) ? a.sqrt_temp * z[i] : 0.0f;
      }
  } else {
    load_rows(lanes, v, a.v, sample);
  }

  for (int i = 0;; ++i) {  // wave-uniform
    EBM_WIDE_STEP_COPIES_OPAQUE();  // smp, hq, key (mlp_wide_rows.h)
    constexpr bool eval_need_energy = true;
#include "mlp_wide_plain_eval.inc"
    // the raw gradient (no clamp: a NaN stays in its chain) and, for i >= 1, the unclamped energy of the counted state
    if (i > 0) {   // the closing B of step i - 1
#pragma unroll
      for (int td = 0; td < DT; ++td)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float vi = v[td][r] - hh * g[td][r];
          v[td][r] = (32 * td + row_of(r, hq) < dim) ? vi : 0.0f;
        }
      if (i > a.burn_in) {  // wave-uniform: step s = i - 1 is counted
        const int j = i - 1 - a.burn_in;
        EBM_WIDE_MOMENTS_COUNT(j);  // second, c, rc, first (mlp_wide_rows.h)
        const Lanes lanes_i{dim, quads, active, hq};  // (the helpers see the opaque K-half)
        const int64_t plane = a.n_chains * (int64_t)dim;
        EBM_WIDE_MOMENTS_PLANES(mom_half, a.mom, 2 * plane);
        moments_rows<false>(lanes_i, mom_half, mom_half + plane, smp, xr, rc, first);
        if (a.v2_mom) {
          EBM_WIDE_MOMENTS_PLANES(v2_half, a.v2_mom, plane);
          moments_rows<true>(lanes_i, v2_half, v2_half, smp, v, rc, first);
        }
        if (a.e_mom) {
          EBM_WIDE_MOMENTS_PLANES(e_half, a.e_mom, 2 * a.n_chains);
          moments_scalar(lanes_i, e_half, e_half + a.n_chains, smp, energy, rc, first);
        }
        const int64_t kept_row = smp * (2 * (int64_t)a.half_len) + j;
        if (a.traj && active) store_rows(lanes_i, a.traj, kept_row, xr);
        if (a.v_traj && active) store_rows(lanes_i, a.v_traj, kept_row, v);
        if (a.e_traj && active && hq == 0) a.e_traj[kept_row] = energy;
      }
    }
    if (i == a.k_steps) break;
    // step i: B, A, O, A -- every operation rounded on its own, a register quad at a time
    const float* noise_i = a.noise ? a.noise + (int64_t)i * a.n_chains * dim : nullptr;
#pragma unroll
    for (int td = 0; td < DT; ++td)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c0 = 32 * td + 8 * q + 4 * hq;
        EBM_WIDE_NOISE_QUAD(z, noise_i, lanes, a.step0 + 1ull + (uint64_t)i);  // (mlp_wide_rows.h)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int r = 4 * q + j;
          float vi = v[td][r] - hh * g[td][r];
          float xv = xr[td][r] + hh * vi;
          vi = c1 * vi + c2 * z[j];
          xv = xv + hh * vi;
          xr[td][r] = (c0 + j < dim) ? xv : 0.0f;
          v[td][r] = (c0 + j < dim) ? vi : 0.0f;
        }
      }
  }
  if (active) {
    store_rows(lanes, a.x, sample, xr);
    store_rows(lanes, a.v, sample, v);
  }
}

struct KineticMomentsWalk {  // (launch_walk_by_dim, mlp_wide_rows.h)
  template <int HT, int DT, int MODE>
  static constexpr auto kernel = &mlp_wide_kinetic_moments_chain<HT, DT, MODE>;
};

}  // namespace widemlp
}  // namespace ebm
