// Kernel body of generalized HMC (Metropolis-adjusted kinetic Langevin) on the wide MLP energy (ebm_ghmc_mlp_chain_f32,
// include/ebm_hip.h; docs/design/ghmc_mlp.md): the transition state machine of mlp_wide_ais_body.h at b = 1 -- mode 0: E and
// dE/dx at the held state, mode 1: after a kick + drift, mode 2: re-evaluation on a scrubbed position, decided per wave -- put
// around the one evaluation (mlp_wide_setup.inc, mlp_wide_eval.inc), with the velocity plane, draw_v0 and the Philox paths of
// mlp_wide_kinetic_body.h.  One wave is 32 chains; position, velocity and force live in the 32x32 C/D layout of the evaluation,
// 16 DT registers each.  Two translation units instantiate it (compiled in parallel): mlp_wide_ghmc.hip (H = 64) and
// mlp_wide_ghmc_h128.hip (H = 128).
//
// The held x and v live in a.x / a.v between transitions; a lane reads back only what it stored itself.  The refreshed velocity
// is stored to a.v in front of the trajectory and that plane is what the flip reads: no fourth register array lives through the
// evaluations.  A transition is n_leapfrog + 1 evaluations and carries no energy or force to the next one (the register argument
// is mlp_wide_ais_body.h's), so the bits do not depend on where a run is cut.
#pragma once
#include "mlp_wide_body.h"

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
  // The images' LDS addresses, formed once: an opaque scalar each (as in mlp_wide_ais_body.h: left visible, the conversion of the
  // LDS pointer is re-derived at its uses inside the evaluation when registers run out, in a form the backend rejects).
  auto walk1_once = walk1;
  auto walk2_once = walk2;
  asm volatile("" : "+s"(walk1_once.base), "+s"(walk2_once.base));

  // rows of a [.., dim] matrix into the C/D layout, zero beyond dim and for the lanes past the last chain (hq: the lane's K-half)
  auto load_rows = [&](float (&dst)[DT][16], const float* src, int64_t row, int hq) {
#pragma unroll
    for (int td = 0; td < DT; ++td)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c0 = 32 * td + 8 * q + 4 * hq;
        if (quads && active && c0 + 3 < dim) {
          const float4 w = *reinterpret_cast<const float4*>(src + row * dim + c0);
          dst[td][4 * q] = w.x; dst[td][4 * q + 1] = w.y; dst[td][4 * q + 2] = w.z; dst[td][4 * q + 3] = w.w;
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) dst[td][4 * q + i] = (active && c0 + i < dim) ? src[row * dim + c0 + i] : 0.0f;
        }
      }
  };
  // (callers guard with `active`; columns past dim never reach memory)
  auto store_rows = [&](float* dst, int64_t row, const float (&src)[DT][16], int hq) {
#pragma unroll
    for (int td = 0; td < DT; ++td)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = 32 * td + row_of(r, hq);
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
  // 0.5 v^T v over the whole chain (both K-halves), clamped to [0, 1e10]
  auto kinetic = [&](const float (&q)[DT][16]) -> float {
    float acc = 0.0f;
#pragma unroll
    for (int td = 0; td < DT; ++td)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc += q[td][r] * q[td][r];
    acc += __shfl_xor(acc, 32);
    return clamp_nanprop(0.5f * acc, 0.0f, 1e10f);
  };

  if (a.draw_v0) {  // wave-uniform: v = sqrt_temp z0, the field at step0; a.v is output only
    float vs[DT][16];
#pragma unroll
    for (int td = 0; td < DT; ++td)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float z[4];
        normal_quad(z, a.key, 32 * td + 8 * q + 4 * h, sample, a.step0);
#pragma unroll
        for (int i = 0; i < 4; ++i) vs[td][4 * q + i] = (32 * td + 8 * q + 4 * h + i < dim) ? a.sqrt_temp * z[i] : 0.0f;
      }
    if (active) store_rows(a.v, sample, vs, h);
  }

  const float eps = a.eps, half_eps = 0.5f * a.eps, c1 = a.c1, c2 = a.c2, beta = a.beta;
  int kept = 0, until_keep = a.thin;
  for (int t = 0; t < a.n_mh; ++t) {  // wave-uniform
    // Nothing derived from the chain index, the lane's K-half or the key is hoisted out of the transition loop and spilled around
    // every evaluation (mlp_wide_kinetic_body.h; docs/design/kinetic_mlp.md).
    int64_t smp = sample;
    int hq = h;
    RngKey key = a.key;
    asm volatile("" : "+v"(smp), "+v"(hq), "+s"(key.k0), "+s"(key.k1));

    // ---- O: the partial refresh, two products and a sum, each rounded on its own, a register quad at a time; the refreshed
    // velocity goes back to a.v, where a reject finds it
    float p[DT][16];
    load_rows(p, a.v, smp, hq);
    {
      const float* noise_t = a.noise ? a.noise + (int64_t)t * a.n_chains * dim : nullptr;
#pragma unroll
      for (int td = 0; td < DT; ++td)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int c0 = 32 * td + 8 * q + 4 * hq;
          float z[4];
          if (noise_t) {
            if (quads && active && c0 + 3 < dim) {
              const float4 w = *reinterpret_cast<const float4*>(noise_t + smp * dim + c0);
              z[0] = w.x; z[1] = w.y; z[2] = w.z; z[3] = w.w;
            } else {
#pragma unroll
              for (int j = 0; j < 4; ++j) z[j] = (active && c0 + j < dim) ? noise_t[smp * dim + c0 + j] : 0.0f;
            }
          } else {
            normal_quad(z, key, c0, smp, a.step0 + 1ull + 2ull * (uint64_t)t);
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float vo = c1 * p[td][4 * q + j] + c2 * z[j];
            p[td][4 * q + j] = (c0 + j < dim) ? vo : 0.0f;
          }
        }
      if (active) store_rows(a.v, smp, p, hq);
    }

    float xr[DT][16], f[DT][16];
    load_rows(xr, a.x, smp, hq);
#pragma unroll
    for (int td = 0; td < DT; ++td)
#pragma unroll
      for (int r = 0; r < 16; ++r) f[td][r] = 0.0f;
    float h0 = 0.0f, e_last = 0.0f;
    int done = 0, mode = 0;  // wave-uniform
    while (done <= a.n_leapfrog) {
      if (mode == 1) {  // first half kick + drift
#pragma unroll
        for (int td = 0; td < DT; ++td)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float ph = __builtin_fmaf(half_eps, f[td][r], p[td][r]);
            p[td][r] = ph;
            const float xn = __builtin_fmaf(eps, ph, xr[td][r]);
            xr[td][r] = (32 * td + row_of(r, hq) < dim) ? xn : 0.0f;
          }
      }
      constexpr bool eval_energy_only = false, eval_block_cuts = false, eval_store_acts = false, eval_need_energy = true, eval_pin = false;
      [[maybe_unused]] float* const act_base = nullptr;
      [[maybe_unused]] constexpr uint32_t act_lane = 0;
      [[maybe_unused]] constexpr float act_seed = 1.0f;
      [[maybe_unused]] const auto eval_aux = [](auto) __attribute__((always_inline)) {};
      [[maybe_unused]] constexpr bool slab_more = true;
      const auto& walk1 = walk1_once;  // (shadow the set-up's: see above)
      const auto& walk2 = walk2_once;
#include "mlp_wide_eval.inc"
      if (mode == 0) {  // H0 and the first (clamped) force, both from this evaluation at the held state
        h0 = clamp_nanprop(energy, -1e10f, 1e10f) + kinetic(p);
#pragma unroll
        for (int td = 0; td < DT; ++td)
#pragma unroll
          for (int r = 0; r < 16; ++r) f[td][r] = clamp_nanprop(-g[td][r], -1e6f, 1e6f);
        e_last = energy;
        mode = 1;
        ++done;
      } else if (mode == 1) {
        // dE/dx at the proposal's position (f is free between the kick above and the force below).  The fast path needs energy
        // and gradient finite in every chain of the wave (a finite E vouches for x, as in mlp_wide_hmc_body.h); decided per
        // WAVE because the literal path re-runs the MFMA evaluation.
        float gz = 0.0f;
#pragma unroll
        for (int td = 0; td < DT; ++td)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float gm = g[td][r];
            f[td][r] = gm;
            gz = __builtin_fmaf(gm, 0.0f, gz);
          }
        const bool all_fine = (bool)__all((__builtin_fabsf(energy) < __builtin_inff()) && gz == 0.0f);
        if (all_fine) {
          float pz = 0.0f;
#pragma unroll
          for (int td = 0; td < DT; ++td)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const float fn = __builtin_amdgcn_fmed3f(-f[td][r], -1e6f, 1e6f);
              const float pn = __builtin_fmaf(half_eps, fn, p[td][r]);
              f[td][r] = fn;
              p[td][r] = pn;
              pz = __builtin_fmaf(pn, 0.0f, pz);
            }
          if (pz != pz) {  // velocity overflow: x is finite, so f stands
#pragma unroll
            for (int td = 0; td < DT; ++td)
#pragma unroll
              for (int r = 0; r < 16; ++r) p[td][r] = nan_to_num0(p[td][r]);
          }
          e_last = energy;
          ++done;
        } else {  // literal semantics: NaN-propagating clamp, scrub, then re-evaluate on the scrubbed x
#pragma unroll
          for (int td = 0; td < DT; ++td)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const float fn = clamp_nanprop(-f[td][r], -1e6f, 1e6f);
              p[td][r] = nan_to_num0(__builtin_fmaf(half_eps, fn, p[td][r]));
              xr[td][r] = nan_to_num0(xr[td][r]);
            }
          mode = 2;
        }
      } else {  // mode 2: force and energy on the scrubbed position
#pragma unroll
        for (int td = 0; td < DT; ++td)
#pragma unroll
          for (int r = 0; r < 16; ++r) f[td][r] = clamp_nanprop(-g[td][r], -1e6f, 1e6f);
        e_last = energy;
        mode = 1;
        ++done;
      }
    }
    // E at the proposal: xr is the position e_last was evaluated at on either path
    const float h1 = clamp_nanprop(e_last, -1e10f, 1e10f) + kinetic(p);

    // ---- Metropolis accept at the temperature T: the Hamiltonian of exp(-E / T) with v ~ N(0, T) is beta (E + K(v))
    const float dlt = clamp_nanprop(beta * (h0 - h1), -50.0f, 50.0f);
    float acc_p = expf(dlt);
    acc_p = (acc_p > 1.0f) ? 1.0f : acc_p;  // NaN stays NaN and rejects
    float uu;
    if (a.u) uu = active ? a.u[(int64_t)t * a.n_chains + smp] : 2.0f;
    else uu = u01_half_open(pick(philox_at(key, (uint64_t)smp >> 2, a.step0 + 2ull + 2ull * (uint64_t)t), (int)(smp & 3)));
    const bool accept = active && (uu < acc_p);
    if (accept) {
      store_rows(a.x, smp, xr, hq);
    } else {  // the flip: the negative of the stored refreshed velocity
      // (read through an opaque copy of the pointer: forwarded from the store above, the plane would live in registers through
      // every evaluation of the trajectory)
      const float* v_plane = a.v;
      asm volatile("" : "+s"(v_plane));
      load_rows(p, v_plane, smp, hq);
#pragma unroll
      for (int td = 0; td < DT; ++td)
#pragma unroll
        for (int r = 0; r < 16; ++r) p[td][r] = -p[td][r];
    }
    if (active) store_rows(a.v, smp, p, hq);
    if (a.accept_mask && active && hq == 0) a.accept_mask[(int64_t)t * a.n_chains + smp] = accept ? 1 : 0;

    if (--until_keep == 0) {  // wave-uniform: (t + 1) % thin == 0
      until_keep = a.thin;
      if (a.traj && kept < a.n_kept) {
        if (!accept) {  // the held position stayed (an opaque pointer again)
          const float* x_plane = a.x;
          asm volatile("" : "+s"(x_plane));
          load_rows(xr, x_plane, smp, hq);
        }
        if (active) store_rows(a.traj, smp * (int64_t)a.n_kept + kept, xr, hq);
      }
      ++kept;
    }
  }
}

template <int HT, int DT>
int launch_ghmc_variant(const WideGhmcArgs& a, hipStream_t st, const char* who) {
  constexpr int MODE = wide_mode(HT, DT);
  const size_t smem = wide_smem_bytes(HT, DT, MODE);
  static DeviceOnce attr_once;  // the LDS opt-in is a per-device function attribute
  if (attr_once.first()) {  // > 64 KiB of dynamic LDS needs the opt-in
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(mlp_wide_ghmc_chain<HT, DT, MODE>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  }
  const int64_t blocks = ceil_div64(a.n_chains, 32 * (kBlock / 64));
  if (blocks > 0x7fffffffLL) return fail(EBM_EINVAL, "%s: too many chains for one launch", who);
  hipLaunchKernelGGL((mlp_wide_ghmc_chain<HT, DT, MODE>), dim3((unsigned)blocks), dim3(kBlock), smem, st, a);
  return check_launch(who);
}

template <int HT>
int launch_ghmc_hidden(const WideGhmcArgs& a, hipStream_t st, const char* who) {
  switch ((a.dim + 31) / 32) {
    case 1: return launch_ghmc_variant<HT, 1>(a, st, who);
    case 2: return launch_ghmc_variant<HT, 2>(a, st, who);
    case 3: return launch_ghmc_variant<HT, 3>(a, st, who);
    default: return launch_ghmc_variant<HT, 4>(a, st, who);
  }
}

}  // namespace widemlp
}  // namespace ebm
