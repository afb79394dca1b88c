// Kernel body of generalized HMC with a scalar or diagonal mass on the wide MLP energy (ebm_ghmc_mlp_chain_mass_f32,
// include/ebm_hip_mass_mlp.h; docs/design/mass_mlp.md): the walk of mlp_wide_ghmc_body.h whose carried plane is the MOMENTUM
// p ~ N(0, T m).  The refresh runs on s_j = c2 m_sqrt_j, the leapfrog drift on eps / m_safe_j, the Hamiltonian on the massed
// kinetic energy K_m (hmc::massed_kinetic's two forms); the kicks, the accept, the flip, rows, noise and Philox coordinates are
// the unit-mass walk's.  The mass forms are LDS tables formed once per workgroup (mlp_wide_mass.h) and read a register quad at a
// time where they are used, through a K-half made opaque at each use: no mass form lives in registers through an evaluation.
// The leapfrog state machine of mlp_wide_leapfrog.inc has no drift hook, so it is spelled here with the massed drift, as
// mlp_wide_hmc_body.h spells its own; the shared text is untouched.  With every factor 1 the kernel computes the unit-mass walk's
// bits.  Two translation units instantiate it: mlp_wide_ghmc_mass.hip (H = 64) and mlp_wide_ghmc_mass_h128.hip (H = 128).
#pragma once
#include "mlp_wide_mass.h"

namespace ebm {
namespace widemlp {

struct WideGhmcMassArgs {
  float* x;              // [n_chains, dim], in/out: the held state
  float* v;              // [n_chains, dim], the momentum plane: in/out, output only with draw_v0
  int64_t n_chains;
  int32_t dim, n_mh, n_leapfrog, thin, n_kept, draw_v0;
  float eps, c1, c2, sqrt_temp, beta;
  int32_t mass_kind;     // EBM_MASS_SCALAR or EBM_MASS_DIAG
  float mass_raw, mass_sqrt, mass_safe;  // scalar mass forms
  const float* mass_diag;                // [dim] or null
  float* traj;           // [n_chains, n_kept, dim] or null
  uint8_t* accept_mask;  // [n_mh, n_chains] or null
  const float* noise;    // [n_mh, n_chains, dim] or null
  const float* u;        // [n_mh, n_chains] or null
  RngKey key;
  uint64_t step0;
  const float* params;
  const char* w1_image;  // always null: the shared set-up text names it for MODE 3, which this kernel is not built for
};

constexpr int kGhmcMassTables = 4;  // eps / m_safe, s = c2 m_sqrt, m_raw, m_sqrt (the start draw's)

// K_m(p) = 0.5 p^T M^-1 p clamped to [0, 1e10], in hmc::massed_kinetic's two forms: per column p^2 / m_raw of a diagonal mass,
// (0.5 sum p^2) / m_raw of a scalar one -- accumulated in kinetic_plain's order (the padding registers are zero and their
// table entries 1).  The K-half is made opaque here: the table's quads are read again at every call.
template <int DT>
__device__ __forceinline__ float kinetic_massed(const float (&q)[DT][16], const float* raw_tab, int hq, bool diag_mass,
                                                float mass_raw) {
  float acc = 0.0f;
  if (diag_mass) {  // wave-uniform
    asm volatile("" : "+v"(hq));
#pragma unroll
    for (int td = 0; td < DT; ++td)
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) {
        float mr[4];
        table_quad(mr, raw_tab, 32 * td + 8 * qd + 4 * hq);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float sq = q[td][4 * qd + j] * q[td][4 * qd + j];
          acc += sq / mr[j];
        }
      }
  } else {
#pragma unroll
    for (int td = 0; td < DT; ++td)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc += q[td][r] * q[td][r];
  }
  acc += __shfl_xor(acc, 32);
  float k = 0.5f * acc;
  if (!diag_mass) k = k / mass_raw;
  return clamp_nanprop(k, 0.0f, 1e10f);
}

template <int HT, int DT, int MODE>
__global__ __launch_bounds__(kBlock, 1) void mlp_wide_ghmc_mass_chain(WideGhmcMassArgs a) {
  static_assert(MODE == 0 || MODE == 2, "weights in LDS: fp32 (0) or split bf16 images (2)");
  constexpr bool EVAL_SCALED = false;
#include "mlp_wide_setup.inc"
  EBM_WIDE_WALKS_ONCE_OPAQUE();  // (mlp_wide_rows.h)
  EBM_WIDE_LANES();

  // the tables, behind the unit-mass layout: 1 at and beyond dim
  float* const drift_tab = wide_smem + wide_smem_bytes(HT, DT, MODE) / sizeof(float);
  float* const refresh_tab = drift_tab + kMassCols;
  float* const raw_tab = refresh_tab + kMassCols;
  float* const sqrt_tab = raw_tab + kMassCols;
  for (int c = threadIdx.x; c < kMassCols; c += kBlock) {
    float m_raw, m_sqrt, m_safe;
    mass_forms_at(a, c, m_raw, m_sqrt, m_safe);
    drift_tab[c] = c < dim ? a.eps / m_safe : 1.0f;
    refresh_tab[c] = c < dim ? a.c2 * m_sqrt : 1.0f;
    raw_tab[c] = m_raw;
    sqrt_tab[c] = m_sqrt;
  }
  __syncthreads();
  const bool diag_mass = a.mass_kind == EBM_MASS_DIAG;  // wave-uniform

  if (a.draw_v0) {  // wave-uniform: p = (sqrt_temp m_sqrt) z0, the field at step0; a.v is output only
    float ps[DT][16];
    draw_momentum(lanes, ps, a, sqrt_tab, sample);
    if (active) store_rows(lanes, a.v, sample, ps);
  }

  const float half_eps = 0.5f * a.eps, c1 = a.c1, beta = a.beta;
  int kept = 0, until_keep = a.thin;
  for (int t = 0; t < a.n_mh; ++t) {  // wave-uniform
    EBM_WIDE_STEP_COPIES_OPAQUE();  // smp, hq, key (mlp_wide_rows.h)
    const Lanes lanes_t{dim, quads, active, hq};  // (the helpers see the opaque K-half)

    // ---- O: the partial refresh p = c1 p + s z, two products and a sum, each rounded on its own, a register quad at a time;
    // the refreshed momentum goes back to a.v, where a reject finds it
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
          float sm[4];
          table_quad(sm, refresh_tab, c0);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float po = c1 * p[td][4 * q + j] + sm[j] * z[j];
            p[td][4 * q + j] = (c0 + j < dim) ? po : 0.0f;
          }
        }
      if (active) store_rows(lanes_t, a.v, smp, p);
    }

    float xr[DT][16];
    load_rows(lanes_t, xr, a.x, smp);

    // ---- the leapfrog trajectory: the state machine of mlp_wide_leapfrog.inc around the one evaluation site, its drift
    // x = fma(eps / m_safe_j, p, x); kicks, clamps and scrubs are that machine's
    float f[DT][16];
#pragma unroll
    for (int td = 0; td < DT; ++td)
#pragma unroll
      for (int r = 0; r < 16; ++r) f[td][r] = 0.0f;
    float h0 = 0.0f, e_last = 0.0f;
    int done = 0, mode = 0;  // wave-uniform
    while (done <= a.n_leapfrog) {
      if (mode == 1) {  // first half kick + drift; the quad's drift scale comes from LDS here, through a K-half made opaque
                        // in this iteration (nothing of the table is carried round the evaluations)
        int hd = hq;
        asm volatile("" : "+v"(hd));
#pragma unroll
        for (int td = 0; td < DT; ++td)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            float dm[4];
            table_quad(dm, drift_tab, 32 * td + 8 * q + 4 * hd);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int r = 4 * q + j;
              const float ph = __builtin_fmaf(half_eps, f[td][r], p[td][r]);
              p[td][r] = ph;
              const float xn = __builtin_fmaf(dm[j], ph, xr[td][r]);
              xr[td][r] = (32 * td + row_of(r, hq) < dim) ? xn : 0.0f;
            }
          }
      }
      constexpr bool eval_need_energy = true;
#include "mlp_wide_plain_eval.inc"
      if (mode == 0) {  // the start Hamiltonian and the first (clamped) force, both from this evaluation at the held state
        h0 = clamp_nanprop(energy, -1e10f, 1e10f) + kinetic_massed<DT>(p, raw_tab, hq, diag_mass, a.mass_raw);
#pragma unroll
        for (int td = 0; td < DT; ++td)
#pragma unroll
          for (int r = 0; r < 16; ++r) f[td][r] = clamp_nanprop(-g[td][r], -1e6f, 1e6f);
        e_last = energy;
        mode = 1;
        ++done;
      } else if (mode == 1) {
        // The gradient at the proposal's position; the fast path needs energy and gradient finite in every chain of the wave,
        // decided per WAVE because the literal path re-runs the MFMA evaluation (mlp_wide_leapfrog.inc).
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
    const float h1 = clamp_nanprop(e_last, -1e10f, 1e10f) + kinetic_massed<DT>(p, raw_tab, hq, diag_mass, a.mass_raw);

    // ---- Metropolis accept at the temperature T: the Hamiltonian of exp(-E / T) with p ~ N(0, T m) is beta (E + K_m(p))
    const float dlt = clamp_nanprop(beta * (h0 - h1), -50.0f, 50.0f);
    float acc_p = expf(dlt);
    acc_p = (acc_p > 1.0f) ? 1.0f : acc_p;  // NaN stays NaN and rejects
    float uu;
    if (a.u) uu = active ? a.u[(int64_t)t * a.n_chains + smp] : 2.0f;
    else uu = u01_half_open(pick(philox_at(key, (uint64_t)smp >> 2, a.step0 + 2ull + 2ull * (uint64_t)t), (int)(smp & 3)));
    const bool accept = active && (uu < acc_p);
    if (accept) {
      store_rows(lanes_t, a.x, smp, xr);
    } else {  // the flip: the negative of the stored refreshed momentum
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

struct GhmcMassWalk {  // (launch_massed_walk_by_dim, mlp_wide_mass.h)
  template <int HT, int DT, int MODE>
  static constexpr auto kernel = &mlp_wide_ghmc_mass_chain<HT, DT, MODE>;
  static constexpr int tables = kGhmcMassTables;
};

}  // namespace widemlp
}  // namespace ebm
