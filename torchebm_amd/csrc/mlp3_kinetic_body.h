// Kernel body of underdamped (kinetic) Langevin dynamics, BAOAB, on the three-hidden-layer SiLU MLP energy at hidden width 64
// (EBM_ENERGY_MLP3, include/ebm_hip_mlp3_kinetic.h; docs/design/mlp3_kinetic.md).  Geometry, LDS and the evaluation are
// mlp3_chain<2, DT>'s (mlp3_body.h): a wave owns 32 chains, a workgroup is four waves, three resident split images and four vectors,
// everything transposed in the 32x32 C/D layout (the set-up is the shared text mlp3_setup.inc, the launch mlp3::launch_kernel);
// mlp3_eval.inc is included ONCE, inside the step loop.  The loop is the one mlp_wide_kinetic_body.h spells for the two-layer
// energy: k_steps + 1 evaluations, evaluation i closes step i - 1 (the B kick, then the kept position) and opens step i
// (B, A, O, A); the two kicks are never merged, so the bits do not depend on where a run is cut.
//
// What lives where across an evaluation (the evaluation alone peaks at 256 VGPRs + 66 / 109 / 187 AGPRs at DT = 1 / 2 / 4):
//   xr  16 DT registers (the evaluation reads it only at its top; the drifts need it behind).
//   v   16 DT registers.
//   g   NOT live: the evaluation declares and writes all of it, the two kicks right behind consume it, and it goes out of scope
//       with the loop body.  No array of draws exists beside the two planes: the update runs a register quad at a time.
#pragma once
#include "mlp3_body.h"

namespace ebm {
namespace mlp3 {

struct KineticArgs {
  float* x;  // [n, dim] in/out
  float* v;  // [n, dim]: in/out, output only with draw_v0
  int64_t n_chains;
  int32_t dim, k_steps, thin, n_kept, draw_v0;
  float hh, c1, c2, sqrt_temp;
  float* traj;         // [n, n_kept, dim] or null
  const float* noise;  // [k_steps, n, dim] or null
  RngKey key;
  uint64_t step0;
  const float* params;  // packed W1[H,dim] b1[H] W2[H,H] b2[H] W3[H,H] b3[H] w4[H] b4[1]
};

template <int DT>
__global__ __launch_bounds__(kBlock, 1) void mlp3_kinetic_chain(KineticArgs a) {
  constexpr int HT = 2;
  constexpr bool B16 = true;
  constexpr bool forward_only = false;
  constexpr int H = 32 * HT, DP = 32 * DT;
  constexpr int C1 = b16_cols(DT);
  constexpr int S1 = DP + 1, S2 = H + 1;  // (the fp32-word branch of the set-up and the evaluation, not instantiated at this width)
#include "mlp3_setup.inc"

  const float hh = a.hh, c1 = a.c1, c2 = a.c2;
  float xr[DT][16], v[DT][16];
  {
    // the start: x, and v given or v = sqrt_temp z0, the normal field at step0, element chain * dim + column
    int64_t smp = sample;  // (opaque here as in the loop: neither row addresses nor column offsets formed here live through it)
    RngKey key = a.key;
    int h0 = h;
    asm volatile("" : "+v"(smp), "+v"(h0), "+s"(key.k0), "+s"(key.k1));
    const Lanes lanes_0{dim, quads, active, h0};
    load_rows(lanes_0, xr, a.x, smp);
    if (a.draw_v0) {  // wave-uniform
      // (the tiles by static_for, here and in the update: sixteen quads with both noise paths and a cut each are more than
      //  `#pragma unroll` takes at DT = 4, and a tile loop left rolled indexes the planes dynamically -- they go to scratch whole)
      mlpb16::static_for<DT>([&](auto tdc) __attribute__((always_inline)) {
        constexpr int td = decltype(tdc)::value;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int c0 = 32 * td + 8 * q + 4 * h0;
          float z[4];
          normal_quad(lanes_0, z, key, c0, smp, a.step0);
#pragma unroll
          for (int j = 0; j < 4; ++j) v[td][4 * q + j] = (c0 + j < dim) ? a.sqrt_temp * z[j] : 0.0f;
          EBM_BLOCK_CUT();  // (a quad's Philox rounds are a block of their own: the scheduler does not run sixteen side by side)
        }
      });
    } else {
      load_rows(lanes_0, v, a.v, smp);
    }
  }

  int until_keep = a.thin;
  int64_t keep_off = 0;
#pragma nounroll
  for (int i = 0;; ++i) {           // wave-uniform
    EBM_WIDE_STEP_COPIES_OPAQUE();  // smp, hq, key (mlp_wide_rows.h): nothing derived from them is hoisted out of the loop
    const Lanes lanes_q{dim, quads, active, hq};
    EBM_BLOCK_CUT();  // (mlp_b16.h: the update in front of and the kicks behind the evaluation are blocks of their own)
#include "mlp3_eval.inc"
    EBM_BLOCK_CUT();
    // The recurrence takes the raw gradient only (no clamp: a NaN stays in its chain) and never the energy.  Its chain through the
    // layer-3 epilogue is left dead: unlike in the two-layer kernel (mlp_wide_kinetic_body.h), the allocation is no worse without
    // it -- 38 / 71 / 190 AGPRs against 68 / 99 / 209 with it kept alive, no scratch either way (docs/design/mlp3_kinetic.md).
    (void)energy;
    if (i > 0) {  // the closing B of step i - 1, then the kept position
#pragma unroll
      for (int td = 0; td < DT; ++td)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float vi = v[td][r] - hh * g[td][r];
          v[td][r] = (32 * td + row_of(r, hq) < dim) ? vi : 0.0f;
        }
      if (--until_keep == 0) {  // i % thin == 0
        until_keep = a.thin;
        if (a.traj && active) store_rows(lanes_q, a.traj + smp * (int64_t)a.n_kept * dim + keep_off, 0, xr);
        keep_off += dim;
      }
    }
    if (i == a.k_steps) break;
    // step i: B, A, O, A -- every operation rounded on its own, a register quad at a time
    const float* noise_i = a.noise ? a.noise + (int64_t)i * a.n_chains * dim : nullptr;
    mlpb16::static_for<DT>([&](auto tdc) __attribute__((always_inline)) {
      constexpr int td = decltype(tdc)::value;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c0 = 32 * td + 8 * q + 4 * hq;
        EBM_WIDE_NOISE_QUAD(z, noise_i, lanes_q, a.step0 + 1ull + (uint64_t)i);  // (mlp_wide_rows.h)
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
        EBM_BLOCK_CUT();
      }
    });
  }
  // Behind the loop the chain index and the K-half are opaque once more: the row addresses and column masks of the stores below
  // are those of the loads above, and left visible they are formed there and live through every evaluation.
  int64_t smp = sample;
  int hs = h;
  asm volatile("" : "+v"(smp), "+v"(hs));
  const Lanes lanes_s{dim, quads, active, hs};
  if (active) {
    store_rows(lanes_s, a.x, smp, xr);
    store_rows(lanes_s, a.v, smp, v);
  }
}

template <int DT>
int launch_kinetic(const KineticArgs& a, hipStream_t st, const char* who) {
  return launch_kernel<&mlp3_kinetic_chain<DT>, 2, DT>(a, st, who);
}

}  // namespace mlp3
}  // namespace ebm
