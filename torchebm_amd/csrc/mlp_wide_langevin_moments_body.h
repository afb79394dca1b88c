// Kernel body of the running moments of overdamped Langevin dynamics, Euler-Maruyama, on the wide MLP energy
// (ebm_chain_moments_mlp_f32, include/ebm_hip.h; docs/design/langevin_moments_mlp.md): the update of ebm_langevin_chain_f32
// without clamp around the plain evaluation of the walks -- ONE evaluation site, the raw gradient, z_s at Philox step step0 + s --
// with the Welford pairs of ebm_chain_moments_f32 beside it.  Two translation units instantiate it (compiled in parallel):
// mlp_wide_langevin_moments.hip (H = 64) and mlp_wide_langevin_moments_h128.hip (H = 128).
//
// Where the pairs live.  In the caller's mom / e_mom planes, as in mlp_wide_kinetic_moments_body.h, updated in place once per
// counted step (moments_rows, mlp_wide_rows.h).  This walk has no velocity, so a plane of means (16 DT registers) could live
// beside the state; it is not kept there: one spelling serves all eight instantiations, the helper and its contract are the ones
// the sibling kernels are tested on, and the position pair is updated right behind the step, when the gradient and everything
// of the evaluation is dead, so nothing of a plane is live through an evaluation and no instantiation has scratch.  The launch
// costs 1.24 - 1.36 of the same steps on the specialised Langevin unit, one more evaluation included (the design note has the
// table); a register-resident mean plane was not measured against it.  A lane reads back only what it stored itself, through an
// opaque copy of the pointer; at c == 1 the planes are not read.  The half switch is a wave-uniform plane offset.
//
// Energies add at most one evaluation.  Evaluation i >= 1 is made at the state behind step i - 1, which is the counted state, so
// its energy is counted behind that evaluation.  With e_mom or e_traj the launch makes k_steps + 1 evaluations (the last one
// for the energy of the final state alone); with neither it makes k_steps: nothing is evaluated behind the last step.
#pragma once
#include "mlp_wide_rows.h"

namespace ebm {
namespace widemlp {

struct WideLangevinMomentsArgs {
  float* x;             // [n_chains, dim], in/out
  int64_t n_chains;
  int32_t dim, k_steps, burn_in, half_len;
  float eta, sqrt_eta, noise_coef;
  const float* recip;   // device [half_len]: float32(1 / c), c = 1 .. half_len
  float* mom;           // [4, n_chains, dim]: mean_a, M2_a, mean_b, M2_b -- working storage during the launch
  float* e_mom;         // [4, n_chains] or null
  float* traj;          // [n_chains, 2 half_len, dim] or null
  float* e_traj;        // [n_chains, 2 half_len] or null
  const float* noise;   // [k_steps, n_chains, dim] or null
  RngKey key;
  uint64_t step0;
  const float* params;
  const char* w1_image;  // always null: the shared set-up text names it for MODE 3, which this kernel is not built for
};

template <int HT, int DT, int MODE>
__global__ __launch_bounds__(kBlock, 1) void mlp_wide_langevin_moments_chain(WideLangevinMomentsArgs a) {
  static_assert(MODE == 0 || MODE == 2, "weights in LDS: fp32 (0) or split bf16 images (2)");
  constexpr bool EVAL_SCALED = false;
#include "mlp_wide_setup.inc"
  EBM_WIDE_WALKS_ONCE_OPAQUE();  // (mlp_wide_rows.h)
  EBM_WIDE_LANES();

  const float eta = a.eta, sqrt_eta = a.sqrt_eta, noise_coef = a.noise_coef;
  const bool want_energy = a.e_mom != nullptr || a.e_traj != nullptr;  // wave-uniform
  float xr[DT][16];
  load_rows(lanes, xr, a.x, sample);

  for (int i = 0;; ++i) {  // wave-uniform
    if (i == a.k_steps && !want_energy) break;  // nothing is evaluated behind the last step
    EBM_WIDE_STEP_COPIES_OPAQUE();  // smp, hq, key (mlp_wide_rows.h)
    constexpr bool eval_need_energy = true;
#include "mlp_wide_plain_eval.inc"
    // the raw gradient (no clamp: a NaN stays in its chain) and, for i >= 1, the unclamped energy of the state behind step i - 1
    if (want_energy && i > a.burn_in) {  // wave-uniform: step s = i - 1 is counted
      const int j = i - 1 - a.burn_in;
      const int64_t kept_row = smp * (2 * (int64_t)a.half_len) + j;
      if (a.e_mom) {
        EBM_WIDE_MOMENTS_COUNT(j);  // second, c, rc, first (mlp_wide_rows.h)
        const Lanes lanes_i{dim, quads, active, hq};  // (the helpers see the opaque K-half)
        EBM_WIDE_MOMENTS_PLANES(e_half, a.e_mom, 2 * a.n_chains);
        moments_scalar(lanes_i, e_half, e_half + a.n_chains, smp, energy, rc, first);
      }
      if (a.e_traj && active && hq == 0) a.e_traj[kept_row] = energy;
    }
    if (i == a.k_steps) break;
    // step i: x1 = x - eta g;  dw = z sqrt_eta;  x' = x1 + noise_coef dw -- every operation rounded on its own, a register quad
    // at a time
    const float* noise_i = a.noise ? a.noise + (int64_t)i * a.n_chains * dim : nullptr;
#pragma unroll
    for (int td = 0; td < DT; ++td)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c0 = 32 * td + 8 * q + 4 * hq;
        EBM_WIDE_NOISE_QUAD(z, noise_i, lanes, a.step0 + (uint64_t)i);  // (mlp_wide_rows.h)
        EBM_WIDE_EULER_MARUYAMA_QUAD();
      }
    if (i >= a.burn_in) {  // wave-uniform: step i is counted, the state behind it
      const int j = i - a.burn_in;
      EBM_WIDE_MOMENTS_COUNT(j);
      const Lanes lanes_i{dim, quads, active, hq};
      const int64_t plane = a.n_chains * (int64_t)dim;
      EBM_WIDE_MOMENTS_PLANES(mom_half, a.mom, 2 * plane);
      moments_rows<false>(lanes_i, mom_half, mom_half + plane, smp, xr, rc, first);
      if (a.traj && active) store_rows(lanes_i, a.traj, smp * (2 * (int64_t)a.half_len) + j, xr);
    }
  }
  if (active) store_rows(lanes, a.x, sample, xr);
}

struct LangevinMomentsWalk {  // (launch_walk_by_dim, mlp_wide_rows.h)
  template <int HT, int DT, int MODE>
  static constexpr auto kernel = &mlp_wide_langevin_moments_chain<HT, DT, MODE>;
};

}  // namespace widemlp
}  // namespace ebm
