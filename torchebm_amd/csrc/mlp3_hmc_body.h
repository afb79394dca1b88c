// Kernel body of the HMC transition on the three-hidden-layer SiLU MLP energy at hidden width 64 (EBM_ENERGY_MLP3,
// include/ebm_hip_mlp3_hmc.h; docs/design/mlp3_hmc.md).  Geometry, LDS and the evaluation are mlp3_chain<2, DT>'s (mlp3_body.h):
// a wave owns 32 chains, a workgroup is four waves, three resident split images and four vectors, everything transposed in the
// 32x32 C/D layout (the set-up is the shared text mlp3_setup.inc, the launch mlp3::launch_kernel); mlp3_eval.inc is included ONCE, inside the leapfrog loop.  The transition is the one mlp_wide_hmc_body.h
// spells for the two-layer energy -- the held position stays in a.x, the mode 0 / 1 / 2 machine with merged kicks, the same
// random field at the same coordinates -- without a diagonal mass and without diagnostics records.
//
// What lives where across an evaluation (the evaluation alone peaks at 256 VGPRs + 66 / 109 / 187 AGPRs at DT = 1 / 2 / 4):
//   xr  16 DT registers, as in mlp3_chain (the evaluation reads it only at its top; the drift needs it behind).
//   p   16 DT registers.
//   f   NOT live: every path behind an evaluation writes all of f before the next kick reads it (the literal path, which
//       has no use for f, zeroes it to say so), so the force costs no register while the contractions run.
#pragma once
#include "mlp3_body.h"

namespace ebm {
namespace mlp3 {

struct HmcArgs {
  float* x;  // [n, dim] in/out: the held position
  int64_t n_chains;
  int32_t dim, n_mh, n_leapfrog;
  float eps;
  const float* eps_table;  // device [n_mh] or null
  int32_t mass_kind;       // EBM_MASS_NONE or EBM_MASS_SCALAR
  float mass_raw, mass_sqrt, mass_safe;
  int32_t thin, n_kept;
  float* traj;  // [n, n_kept, dim] or null
  uint8_t* accept_mask;    // [n_mh, n] or null
  uint32_t* accept_count;  // [n_mh] or null (added to)
  const float* p_noise;    // [n_mh, n, dim] or null
  const float* u;          // [n_mh, n] or null
  RngKey key;
  uint64_t step0;
  const float* params;  // packed W1[H,dim] b1[H] W2[H,H] b2[H] W3[H,H] b3[H] w4[H] b4[1]
};

template <int DT>
__global__ __launch_bounds__(kBlock, 1) void mlp3_hmc_chain(HmcArgs a) {
  constexpr int HT = 2;
  constexpr bool B16 = true;
  constexpr bool forward_only = false;
  constexpr int H = 32 * HT, DP = 32 * DT;
  constexpr int C1 = b16_cols(DT);
  constexpr int S1 = DP + 1, S2 = H + 1;  // (the fp32-word branch of the set-up and the evaluation, not instantiated at this width)
#include "mlp3_setup.inc"

  const bool has_mass = a.mass_kind != EBM_MASS_NONE;
  // 0.5 p^T p [/ m] over the whole chain (both K-halves; the padding registers are zero), clamped to [0, 1e10]
  auto kinetic = [&](const float (&q)[DT][16]) -> float {
    float k = 0.5f * sum_squares<DT>(q);
    if (has_mass) k = k / a.mass_raw;
    return clamp_nanprop(k, 0.0f, 1e10f);
  };

  int until_keep = a.thin;
  int64_t keep_off = 0;
  float eps = a.eps;

  for (int tr = 0; tr < a.n_mh; ++tr) {
    if (a.eps_table) eps = a.eps_table[tr];
    const float half_eps = 0.5f * eps;
    const float em_s = has_mass ? eps / a.mass_safe : eps;  // the drift coefficient eps / max(m, 1e-10)
    int64_t smp = sample;  // nothing derived from the chain index or the key is hoisted out of the transition loop
    RngKey key = a.key;
    int ht = h;  // ... nor from the lane's K-half: the column offsets of the Philox counters, a register pair per element
    asm volatile("" : "+v"(smp), "+v"(ht), "+s"(key.k0), "+s"(key.k1));
    const Lanes lanes_t{dim, quads, active, ht};

    // ---- momentum draw p ~ N(0, m): the normal field at step offset + 2 tr, element chain * dim + column
    float p[DT][16];
    {
      const float* noise_t = a.p_noise ? a.p_noise + (int64_t)tr * a.n_chains * dim : nullptr;
#pragma unroll
      for (int td = 0; td < DT; ++td)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int c0 = 32 * td + 8 * q + 4 * ht;
          EBM_WIDE_NOISE_QUAD(z, noise_t, lanes_t, a.step0 + 2ull * (uint64_t)tr);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            float v = (c0 + i < dim) ? z[i] : 0.0f;
            if (has_mass) v *= a.mass_sqrt;
            p[td][4 * q + i] = v;
          }
          EBM_BLOCK_CUT();  // (a quad's Philox rounds are a block of their own: the scheduler does not run sixteen side by side)
        }
    }

    float xr[DT][16], f[DT][16];
    load_rows(lanes_t, xr, a.x, smp);
#pragma unroll
    for (int td = 0; td < DT; ++td)
#pragma unroll
      for (int r = 0; r < 16; ++r) f[td][r] = 0.0f;
    float h0 = 0.0f, e_last = 0.0f;
    int done = 0, mode = 0;  // wave-uniform
    asm volatile("" : "+s"(mode));  // (opaque: the first pass is not peeled off into a second copy of the evaluation)
#pragma nounroll
    while (done <= a.n_leapfrog) {
      int hq = h;  // the lane's K-half, opaque per evaluation: no column mask lives through the contractions
      asm volatile("" : "+v"(hq));
      if (mode == 1) {  // first half kick + drift
#pragma unroll
        for (int td = 0; td < DT; ++td)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float ph = __builtin_fmaf(half_eps, f[td][r], p[td][r]);
            p[td][r] = ph;
            const float xn = __builtin_fmaf(em_s, ph, xr[td][r]);
            xr[td][r] = (32 * td + row_of(r, hq) < dim) ? xn : 0.0f;
          }
      }
      EBM_BLOCK_CUT();  // (mlp_b16.h: the kick in front of and the epilogues behind the evaluation are blocks of their own)
#include "mlp3_eval.inc"
      EBM_BLOCK_CUT();
      if (mode == 0) {  // H0 and the first (clamped) force
        h0 = clamp_nanprop(energy, -1e10f, 1e10f) + kinetic(p);
#pragma unroll
        for (int td = 0; td < DT; ++td)
#pragma unroll
          for (int r = 0; r < 16; ++r) f[td][r] = clamp_nanprop(-g[td][r], -1e6f, 1e6f);
        e_last = energy;
        mode = 1;
        ++done;
      } else if (mode == 1) {
        // E finite => x finite and the gradient free of NaN; decided per WAVE because the literal path re-runs the evaluation
        const bool all_fine = (bool)__all(__builtin_fabsf(energy) < __builtin_inff());
        if (all_fine) {
          float pz = 0.0f;
#pragma unroll
          for (int td = 0; td < DT; ++td)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const float fn = __builtin_amdgcn_fmed3f(-g[td][r], -1e6f, 1e6f);
              const float pn = __builtin_fmaf(half_eps, fn, p[td][r]);
              f[td][r] = fn;
              p[td][r] = pn;
              pz = __builtin_fmaf(pn, 0.0f, pz);
            }
          if (pz != pz) {  // momentum overflow: x is finite, so f stands
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
              const float fn = clamp_nanprop(-g[td][r], -1e6f, 1e6f);
              p[td][r] = nan_to_num0(__builtin_fmaf(half_eps, fn, p[td][r]));
              xr[td][r] = nan_to_num0(xr[td][r]);
              f[td][r] = 0.0f;  // (mode 2 writes the force: nothing of f lives through the re-evaluation)
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
    const float h1 = clamp_nanprop(e_last, -1e10f, 1e10f) + kinetic(p);

    // Behind the trajectory the chain index and the K-half are opaque once more: the row addresses and column masks of the
    // stores below are those of the loads above, and left visible they are formed there and live through every evaluation.
    int hs = h;
    asm volatile("" : "+v"(smp), "+v"(hs));
    const Lanes lanes_s{dim, quads, active, hs};

    // ---- Metropolis accept: the uniform field at step offset + 2 tr + 1, element chain
    const float dlt = clamp_nanprop(h0 - h1, -50.0f, 50.0f);
    float acc_p = expf(dlt);
    acc_p = (acc_p > 1.0f) ? 1.0f : acc_p;  // clamp_(max=1); NaN stays NaN and rejects
    float uu;
    if (a.u) uu = active ? a.u[(int64_t)tr * a.n_chains + smp] : 2.0f;
    else uu = u01_half_open(pick(philox_at(key, (uint64_t)smp >> 2, a.step0 + 2ull * (uint64_t)tr + 1ull), (int)(smp & 3)));
    const bool accept = active && (uu < acc_p);
    if (accept) store_rows(lanes_s, a.x, smp, xr);
    const bool leader = active && hs == 0;
    if (a.accept_mask && leader) a.accept_mask[(int64_t)tr * a.n_chains + smp] = accept ? 1 : 0;
    if (a.accept_count) {
      const unsigned long long b = __ballot(accept && leader);
      if (lane == 0 && b) atomicAdd(a.accept_count + tr, (uint32_t)__popcll(b));
    }
    if (a.traj && --until_keep == 0) {
      until_keep = a.thin;
      if (active && !accept) load_rows(lanes_s, xr, a.x, smp);  // a rejected chain records the position it stays at
      if (active) store_rows(lanes_s, a.traj + smp * (int64_t)a.n_kept * dim + keep_off, 0, xr);
      keep_off += dim;
    }
  }
}

template <int DT>
int launch_hmc(const HmcArgs& a, hipStream_t st, const char* who) {
  return launch_kernel<&mlp3_hmc_chain<DT>, 2, DT>(a, st, who);
}

}  // namespace mlp3
}  // namespace ebm
