// Kernel body of the running moments of generalized HMC on the wide MLP energy (sampler 1 of ebm_kinetic_moments_mlp_f32,
// include/ebm_hip.h; docs/design/kinetic_moments_mlp.md): the transition of mlp_wide_ghmc_body.h, operation for operation -- the O
// refresh stored back to v, n_leapfrog + 1 evaluations through the safe-mode state machine of mlp_wide_leapfrog.inc, the accept on
// beta (H0 - H1), the flip read from the stored plane, draws at step0 + 1 + 2 t and step0 + 2 + 2 t -- with the Welford pairs of
// ebm_kinetic_moments_f32 beside it.  Two translation units instantiate it (compiled in parallel): mlp_wide_ghmc_moments.hip
// (H = 64) and mlp_wide_ghmc_moments_h128.hip (H = 128).
//
// Where the pairs live.  As the held x and v of the plain body: in the caller's planes (mom, e_mom), updated in place once per
// counted transition (moments_rows, mlp_wide_rows.h) where the plain body keeps its trajectory; a lane reads back only what it
// stored itself, through an opaque copy of the pointer; at c == 1 the planes are not read.  The half switch is a wave-uniform
// plane offset.
//
// The energy of a counted state adds no evaluation: on an accept it is E' of the proposal (e_last of the state machine), on a
// reject the E of the held position that H0 was formed from -- one more register through the trajectory; both unclamped.
#pragma once
#include "mlp_wide_rows.h"

namespace ebm {
namespace widemlp {

struct WideGhmcMomentsArgs {
  float* x;                // [n_chains, dim], in/out: the held state
  float* v;                // [n_chains, dim]: in/out, output only with draw_v0
  int64_t n_chains;
  int32_t dim, k_steps, burn_in, half_len, n_leapfrog, draw_v0;
  float eps, c1, c2, sqrt_temp, beta;
  const float* recip;      // device [half_len]: float32(1 / c), c = 1 .. half_len
  float* mom;              // [4, n_chains, dim]: mean_a, M2_a, mean_b, M2_b -- working storage during the launch
  float* e_mom;            // [4, n_chains] or null
  float* traj;             // [n_chains, 2 half_len, dim] or null
  float* e_traj;           // [n_chains, 2 half_len] or null
  uint8_t* accept_mask;    // [k_steps, n_chains] or null
  uint32_t* accept_count;  // [k_steps] or null: added to
  const float* noise;      // [k_steps, n_chains, dim] or null
  const float* u;          // [k_steps, n_chains] or null
  RngKey key;
  uint64_t step0;
  const float* params;
  const char* w1_image;  // always null: the shared set-up text names it for MODE 3, which this kernel is not built for
};

template <int HT, int DT, int MODE>
__global__ __launch_bounds__(kBlock, 1) void mlp_wide_ghmc_moments_chain(WideGhmcMomentsArgs a) {
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
  for (int t = 0; t < a.k_steps; ++t) {  // wave-uniform
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
    float e_held = 0.0f;  // E at the held position, unclamped: what a reject counts
    const auto leapfrog_grad = [&](int, int, float gr) __attribute__((always_inline)) { return gr; };
    const auto leapfrog_held = [&](float energy) __attribute__((always_inline)) {
      e_held = energy;
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
    } else {  // the flip: the negative of the stored refreshed velocity (an opaque copy of the pointer: mlp_wide_ghmc_body.h)
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
    if (a.accept_count) {  // one ballot and one atomic per wave and transition
      const unsigned long long b = __ballot(accept && hq == 0);
      if ((threadIdx.x & 63) == 0 && b) atomicAdd(a.accept_count + t, (uint32_t)__popcll(b));
    }

    if (t >= a.burn_in) {  // wave-uniform; a rejected proposal counts the held state again
      const int j = t - a.burn_in;
      EBM_WIDE_MOMENTS_COUNT(j);  // second, c, rc, first (mlp_wide_rows.h)
      if (!accept) {  // the held position stayed (an opaque pointer again)
        const float* x_plane = a.x;
        asm volatile("" : "+s"(x_plane));
        load_rows(lanes_t, xr, x_plane, smp);
      }
      const float e_cnt = accept ? e_last : e_held;
      const int64_t plane = a.n_chains * (int64_t)dim;
      EBM_WIDE_MOMENTS_PLANES(mom_half, a.mom, 2 * plane);
      moments_rows<false>(lanes_t, mom_half, mom_half + plane, smp, xr, rc, first);
      if (a.e_mom) {
        EBM_WIDE_MOMENTS_PLANES(e_half, a.e_mom, 2 * a.n_chains);
        moments_scalar(lanes_t, e_half, e_half + a.n_chains, smp, e_cnt, rc, first);
      }
      const int64_t kept_row = smp * (2 * (int64_t)a.half_len) + j;
      if (a.traj && active) store_rows(lanes_t, a.traj, kept_row, xr);
      if (a.e_traj && active && hq == 0) a.e_traj[kept_row] = e_cnt;
    }
  }
}

struct GhmcMomentsWalk {  // (launch_walk_by_dim, mlp_wide_rows.h)
  template <int HT, int DT, int MODE>
  static constexpr auto kernel = &mlp_wide_ghmc_moments_chain<HT, DT, MODE>;
};

}  // namespace widemlp
}  // namespace ebm
