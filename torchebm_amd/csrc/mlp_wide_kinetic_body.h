// Kernel body of underdamped (kinetic) Langevin dynamics, BAOAB, on the wide MLP energy (ebm_kinetic_mlp_chain_f32,
// include/ebm_hip.h; docs/design/kinetic_mlp.md): the walk of kinetic_kernel.h put around the one matrix-core evaluation
// (mlp_wide_setup.inc, mlp_wide_eval.inc) that mlp_wide_hmc_body.h and mlp_wide_ais_body.h put inside their transitions.
// One wave is 32 chains; position, velocity and gradient live in the 32x32 C/D layout of the evaluation, 16 DT registers each,
// and every BAOAB operation is per register: the energy is never needed, so nothing crosses the two K-halves.  Two translation
// units instantiate it (compiled in parallel): mlp_wide_kinetic.hip (H = 64) and mlp_wide_kinetic_h128.hip (H = 128).
//
// The loop has ONE evaluation site and runs k_steps + 1 times: evaluation i closes step i - 1 (the B kick, then the kept
// position) and opens step i (B, A, O, A).  The two kicks are never merged, so the bits do not depend on where a run is cut.
#pragma once
#include "mlp_wide_body.h"

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
  // The images' LDS addresses, formed once: an opaque scalar each (as in mlp_wide_ais_body.h: left visible, the conversion of the
  // LDS pointer is re-derived at its uses inside the evaluation when registers run out, in a form the backend rejects).
  auto walk1_once = walk1;
  auto walk2_once = walk2;
  asm volatile("" : "+s"(walk1_once.base), "+s"(walk2_once.base));

  // rows of a [.., dim] matrix into the C/D layout, zero beyond dim and for the lanes past the last chain
  auto load_rows = [&](float (&dst)[DT][16], const float* src, int64_t row) {
#pragma unroll
    for (int td = 0; td < DT; ++td)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c0 = 32 * td + 8 * q + 4 * h;
        if (quads && active && c0 + 3 < dim) {
          const float4 w = *reinterpret_cast<const float4*>(src + row * dim + c0);
          dst[td][4 * q] = w.x; dst[td][4 * q + 1] = w.y; dst[td][4 * q + 2] = w.z; dst[td][4 * q + 3] = w.w;
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) dst[td][4 * q + i] = (active && c0 + i < dim) ? src[row * dim + c0 + i] : 0.0f;
        }
      }
  };
  auto store_rows = [&](float* dst, int64_t row, const float (&src)[DT][16]) {
#pragma unroll
    for (int td = 0; td < DT; ++td)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = 32 * td + row_of(r, h);
        if (c < dim) dst[row * dim + c] = src[td][r];
      }
  };
  // one register quad of the normal field at `step`, element chain * dim + col (zero beyond dim): one Philox counter where a
  // quad is four aligned columns, per element otherwise
  auto normal_quad = [&](float (&z)[4], RngKey key, int c0, int64_t row, uint64_t step) {
#pragma unroll
    for (int i = 0; i < 4; ++i) z[i] = 0.0f;
    if (c0 < dim) {
      if (quads) {
        const F4 nrm = normal4_at(key, ((uint64_t)row * (uint64_t)dim + (uint64_t)c0) >> 2, step);
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
            nrm = normal4_at(key, have, step);
          }
          const int w = (int)(e & 3);
          z[i] = w == 0 ? nrm.v[0] : (w == 1 ? nrm.v[1] : (w == 2 ? nrm.v[2] : nrm.v[3]));
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) z[i] = (c0 + i < dim) ? z[i] : 0.0f;
  };

  const float hh = a.hh, c1 = a.c1, c2 = a.c2;
  float xr[DT][16], v[DT][16];
  load_rows(xr, a.x, sample);
  if (a.draw_v0) {  // wave-uniform: v = sqrt_temp z0, the field at step0
#pragma unroll
    for (int td = 0; td < DT; ++td)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float z[4];
        normal_quad(z, a.key, 32 * td + 8 * q + 4 * h, sample, a.step0);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[td][4 * q + i] = (32 * td + 8 * q + 4 * h + i < dim) ? a.sqrt_temp * z[i] : 0.0f;
      }
  } else {
    load_rows(v, a.v, sample);
  }

  int kept = 0, until_keep = a.thin;
  for (int i = 0;; ++i) {  // wave-uniform
    // Nothing derived from the chain index, the lane's K-half or the key is hoisted out of the step loop and spilled around
    // every evaluation: left invariant, the 64-bit column offsets of the Philox counters (a register pair per element), the
    // column masks (a scalar pair each) and the round keys are all formed in front of the loop and live through it.
    int64_t smp = sample;
    int hq = h;
    RngKey key = a.key;
    asm volatile("" : "+v"(smp), "+v"(hq), "+s"(key.k0), "+s"(key.k1));
    constexpr bool eval_energy_only = false, eval_block_cuts = false, eval_store_acts = false, eval_need_energy = false, eval_pin = false;
    [[maybe_unused]] float* const act_base = nullptr;
    [[maybe_unused]] constexpr uint32_t act_lane = 0;
    [[maybe_unused]] constexpr float act_seed = 1.0f;
    [[maybe_unused]] const auto eval_aux = [](auto) __attribute__((always_inline)) {};
    [[maybe_unused]] constexpr bool slab_more = true;
    const auto& walk1 = walk1_once;  // (shadow the set-up's: see above)
    const auto& walk2 = walk2_once;
#include "mlp_wide_eval.inc"
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
        if (a.traj && kept < a.n_kept && active) store_rows(a.traj, smp * (int64_t)a.n_kept + kept, xr);
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
        float z[4];
        if (noise_i) {
          if (quads && active && c0 + 3 < dim) {
            const float4 w = *reinterpret_cast<const float4*>(noise_i + smp * dim + c0);
            z[0] = w.x; z[1] = w.y; z[2] = w.z; z[3] = w.w;
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) z[j] = (active && c0 + j < dim) ? noise_i[smp * dim + c0 + j] : 0.0f;
          }
        } else {
          normal_quad(z, key, c0, smp, a.step0 + 1ull + (uint64_t)i);
        }
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
    store_rows(a.x, sample, xr);
    store_rows(a.v, sample, v);
  }
}

template <int HT, int DT>
int launch_kinetic_variant(const WideKineticArgs& a, hipStream_t st, const char* who) {
  constexpr int MODE = wide_mode(HT, DT);
  const size_t smem = wide_smem_bytes(HT, DT, MODE);
  static DeviceOnce attr_once;  // the LDS opt-in is a per-device function attribute
  if (attr_once.first()) {  // > 64 KiB of dynamic LDS needs the opt-in
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(mlp_wide_kinetic_chain<HT, DT, MODE>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  }
  const int64_t blocks = ceil_div64(a.n_chains, 32 * (kBlock / 64));
  if (blocks > 0x7fffffffLL) return fail(EBM_EINVAL, "%s: too many chains for one launch", who);
  hipLaunchKernelGGL((mlp_wide_kinetic_chain<HT, DT, MODE>), dim3((unsigned)blocks), dim3(kBlock), smem, st, a);
  return check_launch(who);
}

template <int HT>
int launch_kinetic_hidden(const WideKineticArgs& a, hipStream_t st, const char* who) {
  switch ((a.dim + 31) / 32) {
    case 1: return launch_kinetic_variant<HT, 1>(a, st, who);
    case 2: return launch_kinetic_variant<HT, 2>(a, st, who);
    case 3: return launch_kinetic_variant<HT, 3>(a, st, who);
    default: return launch_kinetic_variant<HT, 4>(a, st, who);
  }
}

}  // namespace widemlp
}  // namespace ebm
