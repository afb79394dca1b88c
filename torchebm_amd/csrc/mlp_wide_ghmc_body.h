// Kernel body of generalized HMC (Metropolis-adjusted kinetic Langevin) on the wide MLP energy (ebm_ghmc_mlp_chain_f32,
// include/ebm_hip.h; docs/design/ghmc_mlp.md): the refresh, the flip and the accept put around the shared leapfrog state machine
// (mlp_wide_leapfrog.inc, with the plain gradient and H0 = E + K as its hooks) and through it around the one evaluation
// (mlp_wide_setup.inc, mlp_wide_eval.inc); rows, noise and the launch are mlp_wide_rows.h's.  One wave is 32 chains; position,
// velocity and force live in the 32x32 C/D layout of the evaluation, 16 DT registers each.  Two translation units instantiate
// it (compiled in parallel): mlp_wide_ghmc.hip (H = 64) and mlp_wide_ghmc_h128.hip (H = 128).
//
// The held x and v live in a.x / a.v between transitions; a lane reads back only what it stored itself.  The refreshed velocity
// is stored to a.v in front of the trajectory and that plane is what the flip reads: no fourth register array lives through the
// evaluations.  A transition is n_leapfrog + 1 evaluations and carries no energy or force to the next one (16 DT + 1 more live
// registers per lane through every evaluation, in kernels at the register limit), so the bits do not depend on where a run is cut.
#pragma once
#include "mlp_wide_rows.h"

namespace ebm {
namespace widemlp {

struct WideGhmcArgs {
  float* x;              // [n_chains, dim], in/out: the held state
  float* v;              // [n_chains, dim]: in/out, output only with draw_v0
  int64_t n_chains;
  int32_t dim, n_mh, n_leapfrog, thin, n_kept, draw_v0;
  float eps, c1, c2, sqrt_temp, beta;
  float* traj;           // [n_chains, n_kept, dim] or null
  uint8_t* accept_mask;  // [n_mh, n_chains] or null
  const float* noise;    // [n_mh, n_chains, dim] or null
  const float* u;        // [n_mh, n_chains] or null
  RngKey key;
  uint64_t step0;
  const float* params;
  const char* w1_image;  // always null: the shared set-up text names it for MODE 3, which this kernel is not built for
};

template <int HT, int DT, int MODE>
__global__ __launch_bounds__(kBlock, 1) void mlp_wide_ghmc_chain(WideGhmcArgs a) {
  static_assert(MODE == 0 || MODE == 2, "weights in LDS: fp32 (0) or split bf16 images (2)");
  constexpr bool EVAL_SCALED = false;
#include "mlp_wide_setup.inc"
  EBM_WIDE_WALKS_ONCE_OPAQUE();  // (mlp_wide_rows.h)
  EBM_WIDE_LANES();

  if (a.draw_v0) {  // wave-uniform: v = sqrt_temp z0, the field at step0; a.v is output only
    float vs[DT][16];
#pragma unroll
    for (int td = 0; td < DT; ++td)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float z[4];
        normal_quad(lanes, z, a.key, 32 * td + 8 * q + 4 * h, sample, a.step0);
#pragma unroll
        for (int i = 0; i < 4; ++i) vs[td][4 * q + i] = (32 * td + 8 * q + 4 * h + i < dim) ? a.sqrt_temp * z[i] : 0.0f;
      }
    if (active) store_rows(lanes, a.v, sample, vs);
  }

  const float eps = a.eps, half_eps = 0.5f * a.eps, c1 = a.c1, c2 = a.c2, beta = a.beta;
  int kept = 0, until_keep = a.thin;
  for (int t = 0; t < a.n_mh; ++t) {  // wave-uniform
    EBM_WIDE_STEP_COPIES_OPAQUE();  // smp, hq, key (mlp_wide_rows.h)
    const Lanes lanes_t{dim, quads, active, hq};  // (the helpers see the opaque K-half)

    // ---- O: the partial refresh, two products and a sum, each rounded on its own, a register quad at a time; the refreshed
    // velocity goes back to a.v, where a reject finds it
    float p[DT][16];
    load_rows(lanes_t, p, a.v, smp);
    {
      const float* noise_t = a.noise ? a.noise + (int64_t)t * a.n_chains * dim : nullptr;
#pragma unroll
      for (int td = 0; td < DT; ++td)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int c0 = 32 * td + 8 * q + 4 * hq;
          EBM_WIDE_NOISE_QUAD(z, noise_t, lanes_t, a.step0 + 1ull + 2ull * (uint64_t)t);  // (mlp_wide_rows.h)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float vo = c1 * p[td][4 * q + j] + c2 * z[j];
            p[td][4 * q + j] = (c0 + j < dim) ? vo : 0.0f;
          }
        }
      if (active) store_rows(lanes_t, a.v, smp, p);
    }

    float xr[DT][16];
    load_rows(lanes_t, xr, a.x, smp);
    const auto leapfrog_grad = [&](int, int, float gr) __attribute__((always_inline)) { return gr; };
    const auto leapfrog_held = [&](float energy) __attribute__((always_inline)) {
      return clamp_nanprop(energy, -1e10f, 1e10f) + kinetic_plain<DT>(p);
    };
#include "mlp_wide_leapfrog.inc"
    // E at the proposal: xr is the position e_last was evaluated at on either path
    const float h1 = clamp_nanprop(e_last, -1e10f, 1e10f) + kinetic_plain<DT>(p);

    // ---- Metropolis accept at the temperature T: the Hamiltonian of exp(-E / T) with v ~ N(0, T) is beta (E + K(v))
    const float dlt = clamp_nanprop(beta * (h0 - h1), -50.0f, 50.0f);
    float acc_p = expf(dlt);
    acc_p = (acc_p > 1.0f) ? 1.0f : acc_p;  // NaN stays NaN and rejects
    float uu;
    if (a.u) uu = active ? a.u[(int64_t)t * a.n_chains + smp] : 2.0f;
    else uu = u01_half_open(pick(philox_at(key, (uint64_t)smp >> 2, a.step0 + 2ull + 2ull * (uint64_t)t), (int)(smp & 3)));
    const bool accept = active && (uu < acc_p);
    if (accept) {
      store_rows(lanes_t, a.x, smp, xr);
    } else {  // the flip: the negative of the stored refreshed velocity
      // (read through an opaque copy of the pointer: forwarded from the store above, the plane would live in registers through
      // every evaluation of the trajectory)
      const float* v_plane = a.v;
      asm volatile("" : "+s"(v_plane));
      load_rows(lanes_t, p, v_plane, smp);
#pragma unroll
      for (int td = 0; td < DT; ++td)
#pragma unroll
        for (int r = 0; r < 16; ++r) p[td][r] = -p[td][r];
    }
    if (active) store_rows(lanes_t, a.v, smp, p);
    if (a.accept_mask && active && hq == 0) a.accept_mask[(int64_t)t * a.n_chains + smp] = accept ? 1 : 0;

    if (--until_keep == 0) {  // wave-uniform: (t + 1) % thin == 0
      until_keep = a.thin;
      if (a.traj && kept < a.n_kept) {
        if (!accept) {  // the held position stayed (an opaque pointer again)
          const float* x_plane = a.x;
          asm volatile("" : "+s"(x_plane));
          load_rows(lanes_t, xr, x_plane, smp);
        }
        if (active) store_rows(lanes_t, a.traj, smp * (int64_t)a.n_kept + kept, xr);
      }
      ++kept;
    }
  }
}

struct GhmcWalk {  // (launch_walk_by_dim, mlp_wide_rows.h)
  template <int HT, int DT, int MODE>
  static constexpr auto kernel = &mlp_wide_ghmc_chain<HT, DT, MODE>;
};

}  // namespace widemlp
}  // namespace ebm
