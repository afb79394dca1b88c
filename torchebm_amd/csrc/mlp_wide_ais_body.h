// Kernel body of annealed importance sampling on the wide MLP energy (ebm_ais_mlp_chain_f32, include/ebm_hip.h;
// docs/design/ais_mlp.md): the ladder, the momentum draw, the accept and the chain's importance weight (a Kahan pair) put around
// the shared leapfrog state machine (mlp_wide_leapfrog.inc) walking the PATH energy
//   U_b(x) = (1 - b) E_0(x) + b E(x),   E_0(x) = 0.5 inv_var0 sum x^2
// and through it around the one evaluation (mlp_wide_setup.inc, mlp_wide_eval.inc); rows, noise and the launch are
// mlp_wide_rows.h's.  One wave is 32 chains; state, momentum and force live in the 32x32 C/D layout of the evaluation.  Two
// translation units instantiate it (compiled in parallel): mlp_wide_ais.hip (H = 64) and mlp_wide_ais_h128.hip (H = 128).
//
// A transition is n_leapfrog + 1 evaluations, as the HMC sibling's: the mode-0 evaluation at the top of step t is where the weight
// update takes E(x) from.  (Carrying E and the raw gradient of an accepted proposal to the next step would save it, at 16 DT + 1
// more live registers per lane through every evaluation, in kernels that are at the register limit already.)
// The mix is (1 - b) * a + b * c in separately rounded operations, never divided by b: at b = 1 it is 0 * a + 1 * c = c, and the
// transition is mlp_wide_hmc_kernel's (general variant, identity mass) bit for bit.
#pragma once
#include "mlp_wide_rows.h"

namespace ebm {
namespace widemlp {

struct WideAisArgs {
  float* x;                 // [n_chains, dim]: the held state; written before it is read, the final states at the end
  float* logw;              // [n_chains]
  int64_t n_chains;
  int32_t dim, n_temps, n_leapfrog;
  const float* beta;        // device [n_temps + 1]
  const float* eps;         // device [n_temps]
  float sigma0, inv_var0;
  uint8_t* accept_mask;     // [n_temps, n_chains] or null
  uint32_t* accept_counts;  // [n_temps] or null
  const float* x0;          // [n_chains, dim] or null
  const float* p_noise;     // [n_temps, n_chains, dim] or null
  const float* u_accept;    // [n_temps, n_chains] or null
  RngKey key;
  uint64_t step0;
  const float* params;
  const char* w1_image;     // always null: the shared set-up text names it for MODE 3, which this kernel is not built for
};

template <int HT, int DT, int MODE>
__global__ __launch_bounds__(kBlock, 1) void mlp_wide_ais_chain(WideAisArgs a) {
  static_assert(MODE == 0 || MODE == 2, "weights in LDS: fp32 (0) or split bf16 images (2)");
  constexpr bool EVAL_SCALED = false;
#include "mlp_wide_setup.inc"
  EBM_WIDE_WALKS_ONCE_OPAQUE();  // (mlp_wide_rows.h)
  EBM_WIDE_LANES();
  const int& hq = h;  // the lane's K-half as the shared text names it (not opaque in this kernel)

  // Three helpers this kernel keeps in its own words -- the field is normal_quad's, the store store_rows', the sum sum_squares' of
  // mlp_wide_rows.h: through those, with the shared loop, the H = 128, dim 33 .. 64 kernel takes 8 bytes more scratch (200 -> 208,
  // two more spills); spelled here no kernel of the family spills more than it did (docs/design/mlp_wide.md).
  // the normal field at `step`, element chain * dim + col, in the C/D layout (zero beyond dim): per quad where a register quad is
  // one Philox counter, per element otherwise
  auto normal_rows = [&](float (&dst)[DT][16], int64_t row, uint64_t step) {
#pragma unroll
    for (int td = 0; td < DT; ++td)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c0 = 32 * td + 8 * q + 4 * h;
        float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (c0 < dim) {
          if (quads) {
            const F4 nrm = normal4_at(a.key, ((uint64_t)row * (uint64_t)dim + (uint64_t)c0) >> 2, step);
#pragma unroll
            for (int i = 0; i < 4; ++i) z[i] = nrm.v[i];
          } else {
            uint64_t have = ~0ull;
            F4 nrm;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const uint64_t e = (uint64_t)row * (uint64_t)dim + (uint64_t)(c0 + i);
              if ((e >> 2) != have) {
                have = e >> 2;
                nrm = normal4_at(a.key, have, step);
              }
              const int w = (int)(e & 3);
              z[i] = w == 0 ? nrm.v[0] : (w == 1 ? nrm.v[1] : (w == 2 ? nrm.v[2] : nrm.v[3]));
            }
          }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) dst[td][4 * q + i] = (c0 + i < dim) ? z[i] : 0.0f;
      }
  };
  // the held state lives in a.x between transitions (as in mlp_wide_hmc_body.h); a lane reads back only what it stored itself
  auto store_state = [&](const float (&src)[DT][16], int64_t row) {
#pragma unroll
    for (int td = 0; td < DT; ++td)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = 32 * td + row_of(r, h);
        if (c < dim) a.x[row * dim + c] = src[td][r];
      }
  };
  // E_0 = 0.5 inv_var0 sum x^2 (the padding registers are zero)
  const float half_inv_var0 = 0.5f * a.inv_var0;
  auto base_energy = [&](const float (&q)[DT][16]) -> float {
    float acc = 0.0f;
#pragma unroll
    for (int td = 0; td < DT; ++td)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc += q[td][r] * q[td][r];
    acc += __shfl_xor(acc, 32);
    return half_inv_var0 * acc;
  };

  // ---- start: the injected state, or sigma0 z
  {
    float xs[DT][16];
    if (a.x0) {
      load_rows(lanes, xs, a.x0, sample);
    } else {
      normal_rows(xs, sample, a.step0);
#pragma unroll
      for (int td = 0; td < DT; ++td)
#pragma unroll
        for (int r = 0; r < 16; ++r) xs[td][r] = (32 * td + row_of(r, h) < dim) ? a.sigma0 * xs[td][r] : 0.0f;
    }
    if (active) store_state(xs, sample);
  }

  float lw = 0.0f, lw_c = 0.0f;  // the weight: a Kahan pair
  float beta_prev = a.beta[0];

  for (int t = 1; t <= a.n_temps; ++t) {
    const float beta_t = a.beta[t];  // wave-uniform
    const float eps = a.eps[t - 1];
    const float half_eps = 0.5f * eps;
    const float db = beta_t - beta_prev, b0 = 1.0f - beta_t, c0 = b0 * a.inv_var0;
    beta_prev = beta_t;
    int64_t smp = sample;  // nothing derived from the chain index is hoisted out of the step loop and spilled
    asm volatile("" : "+v"(smp));

    // ---- momentum draw p ~ N(0, I)
    float p[DT][16];
    if (a.p_noise) load_rows(lanes, p, a.p_noise + (int64_t)(t - 1) * a.n_chains * dim, smp);
    else normal_rows(p, smp, a.step0 + 2ull * (uint64_t)t - 1ull);

    float xr[DT][16];
    load_rows(lanes, xr, a.x, smp);
    // dU/dx = (1 - b) inv_var0 x + b dE/dx
    const auto leapfrog_grad = [&](int td, int r, float gr) __attribute__((always_inline)) { return c0 * xr[td][r] + beta_t * gr; };
    // the evaluation at the held state: the weight, then H0
    const auto leapfrog_held = [&](float energy) __attribute__((always_inline)) {
      const float e0 = base_energy(xr);
      const float term = db * (e0 - energy);
      const float y = term - lw_c;
      const float s = lw + y;
      lw_c = (__builtin_fabsf(s) < __builtin_inff()) ? (s - lw) - y : 0.0f;  // an infinite sum stays what a plain sum gives
      lw = s;
      return clamp_nanprop(b0 * e0 + beta_t * energy, -1e10f, 1e10f) + kinetic_plain<DT>(p);
    };
#include "mlp_wide_leapfrog.inc"
    // U at the proposal: xr is the position e_last was evaluated at on either path
    const float h1 = clamp_nanprop(b0 * base_energy(xr) + beta_t * e_last, -1e10f, 1e10f) + kinetic_plain<DT>(p);

    // ---- Metropolis accept
    const float dlt = clamp_nanprop(h0 - h1, -50.0f, 50.0f);
    float acc_p = expf(dlt);
    acc_p = (acc_p > 1.0f) ? 1.0f : acc_p;  // NaN stays NaN and rejects
    float uu;
    if (a.u_accept) uu = active ? a.u_accept[(int64_t)(t - 1) * a.n_chains + smp] : 2.0f;
    else uu = u01_half_open(pick(philox_at(a.key, (uint64_t)smp >> 2, a.step0 + 2ull * (uint64_t)t), (int)(smp & 3)));
    const bool accept = active && (uu < acc_p);
    if (accept) store_state(xr, smp);
    const bool leader = active && h == 0;
    if (a.accept_mask && leader) a.accept_mask[(int64_t)(t - 1) * a.n_chains + smp] = accept ? 1 : 0;
    if (a.accept_counts) {  // one ballot and one atomic per wave and temperature
      const unsigned long long b = __ballot(accept && leader);
      if (lane == 0 && b) atomicAdd(a.accept_counts + (t - 1), (uint32_t)__popcll(b));
    }
  }
  if (active && h == 0) a.logw[sample] = lw;
}

struct AisWalk {  // (launch_walk_by_dim, mlp_wide_rows.h)
  template <int HT, int DT, int MODE>
  static constexpr auto kernel = &mlp_wide_ais_chain<HT, DT, MODE>;
};

}  // namespace widemlp
}  // namespace ebm
