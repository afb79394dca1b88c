// Kernel body of underdamped (kinetic) Langevin dynamics, BAOAB, on the wide MLP energy (ebm_kinetic_mlp_chain_f32,
// include/ebm_hip.h; docs/design/kinetic_mlp.md): the walk of kinetic_kernel.h put around the one matrix-core evaluation
// (mlp_wide_setup.inc, mlp_wide_eval.inc) that the Metropolis-corrected walks put inside their transitions; rows, noise, the
// plain-evaluation preamble and the launch are mlp_wide_rows.h's.  One wave is 32 chains; position, velocity and gradient live
// in the 32x32 C/D layout of the evaluation, 16 DT registers each, and every BAOAB operation is per register: the energy is
// never needed, so nothing crosses the two K-halves.  Two translation units instantiate it (compiled in parallel):
// mlp_wide_kinetic.hip (H = 64) and mlp_wide_kinetic_h128.hip (H = 128).
//
// The loop has ONE evaluation site and runs k_steps + 1 times: evaluation i closes step i - 1 (the B kick, then the kept
// position) and opens step i (B, A, O, A).  The two kicks are never merged, so the bits do not depend on where a run is cut.
#pragma once
#include "mlp_wide_rows.h"

namespace ebm {
namespace widemlp {

struct WideKineticArgs {
  float* x;             // [n_chains, dim], in/out
  float* v;             // [n_chains, dim]: in/out, output only with draw_v0
  int64_t n_chains;
  int32_t dim, k_steps, thin, n_kept, draw_v0;
  float hh, c1, c2, sqrt_temp;
  float* traj;          // [n_chains, n_kept, dim] or null
  const float* noise;   // [k_steps, n_chains, dim] or null
  RngKey key;
  uint64_t step0;
  const float* params;
  const char* w1_image;  // always null: the shared set-up text names it for MODE 3, which this kernel is not built for
};

template <int HT, int DT, int MODE>
__global__ __launch_bounds__(kBlock, 1) void mlp_wide_kinetic_chain(WideKineticArgs a) {
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

  int kept = 0, until_keep = a.thin;
  for (int i = 0;; ++i) {  // wave-uniform
    EBM_WIDE_STEP_COPIES_OPAQUE();  // smp, hq, key (mlp_wide_rows.h)
    constexpr bool eval_need_energy = false;
#include "mlp_wide_plain_eval.inc"
    // The recurrence takes the raw gradient only (no clamp: a NaN stays in its chain) and never the energy.  The energy's chain of
    // 16 HT FMAs through the layer-2 epilogue (and its one cross-half shuffle) is kept alive all the same, by a use that issues
    // nothing: with the chain dead the compiler schedules the evaluation differently and it alone overflows the register file
    // -- measured at H = 128, dim <= 32: 256 AGPRs and 556 bytes of scratch per lane, against 138 AGPRs and none with it alive
    // (docs/design/kinetic_mlp.md).
    asm volatile("" ::"v"(energy));
    if (i > 0) {   // the closing B of step i - 1
#pragma unroll
      for (int td = 0; td < DT; ++td)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float vi = v[td][r] - hh * g[td][r];
          v[td][r] = (32 * td + row_of(r, hq) < dim) ? vi : 0.0f;
        }
      if (--until_keep == 0) {  // i % thin == 0
        until_keep = a.thin;
        if (a.traj && kept < a.n_kept && active) store_rows(lanes, a.traj, smp * (int64_t)a.n_kept + kept, xr);
        ++kept;
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

struct KineticWalk {  // (launch_walk_by_dim, mlp_wide_rows.h)
  template <int HT, int DT, int MODE>
  static constexpr auto kernel = &mlp_wide_kinetic_chain<HT, DT, MODE>;
};

}  // namespace widemlp
}  // namespace ebm
