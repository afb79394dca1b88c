// Shared pieces of the element-wise Langevin chain kernels (langevin.hip: the plain variants,
// langevin_diag.hip: the variants that also emit diagnostics records): update arithmetic, gradient
// folds, vector load / store helpers, launch arguments and the lean k-fused kernel template.
#pragma once
#include <cmath>

#include "chain_launch.h"

namespace ebm {

// langevin_fold.hip: the folded DoubleWell loop on plain f32 instructions (lean_body PLAIN), in a unit of its own for its compile
// flag.  The caller has checked lean_fold_ok (fold_eta = its E) and the grid; c64 = !lean_counters32.
int langevin_lean_fold_plain_launch(const LangevinChainReq& q, float fold_eta, bool c64, unsigned blocks, hipStream_t st);

namespace {

constexpr int kBlock = 256;  // 4 waves: one per SIMD of a CU
// The lean kernels' energy-kind value for the folded DoubleWell loop (lean_body FOLD).  Internal: the launcher picks it for
// DoubleWell calls that meet lean_fold_ok; it is no ebm_energy_t and no caller passes it.
constexpr int kDoubleWellFold = 16;
// ... and the same loop on plain f32 instructions (lean_body PLAIN; langevin_fold.hip): what the launcher takes for those calls.
// Kind 16 stays the A/B route (EBM_NO_LEAN_PLAIN) and the form tests/test_isa_lean_fold.py pins.
constexpr int kDoubleWellFoldPlain = 17;

typedef float v2f __attribute__((ext_vector_type(2)));

struct StepCoef {
  float eta, sqrt_eta, noise_coef;
};

// Reference arithmetic for one element (core/base_integrator.py:397,728-729), each op
// rounded separately:  x + eta*(1.0*(-g))  ==  x - fl(eta*g)  bit for bit.
__device__ __forceinline__ float em_update(float x, float g, float eps, StepCoef c) {
  const float x1 = x - c.eta * g;
  const float dw = eps * c.sqrt_eta;
  return x1 + c.noise_coef * dw;
}

// Gradients with autograd's rounding.  Autograd evaluates (h*(2u))*(2x) and
// (0.5k)*(2x); scaling by 2 is exact and commutes with rounding, so fl(fl(h*2u)*2x) == fl(fl(4h*u)*x)
// and fl(s*2x) == fl(2s*x) bit for bit (overflow included: both sides reach inf together; the
// intermediate never lies in the denormal range).  The doubled constants are wave-uniform: two
// multiplies per element instead of four (DoubleWell), one instead of two (Harmonic).
template <int KIND>
__device__ __forceinline__ float elem_grad(float x, float s0, float s1) {
  if constexpr (KIND == EBM_ENERGY_DOUBLE_WELL) {
    const float u = x * x - s1;                // x.pow(2) - b**2
    return ((4.0f * s0) * u) * x;              // == (h*(2u)) * (2x), pow backward twice
  } else {
    return (2.0f * s0) * x;                    // == (0.5k) * (2x)
  }
}

__device__ __forceinline__ F4 load4(const float* __restrict__ p, int64_t e0, int n_valid, bool vec) {
  F4 r;
  if (vec && n_valid == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p + e0);
    r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) r.v[i] = (i < n_valid) ? p[e0 + i] : 0.0f;
  }
  return r;
}

__device__ __forceinline__ void store4(float* __restrict__ p, int64_t e0, int n_valid, bool vec, F4 r) {
  if (vec && n_valid == 4) {
    *reinterpret_cast<float4*>(p + e0) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < n_valid) p[e0 + i] = r.v[i];
  }
}

// ---------------------------------------------------------------------------------
// k-fused chain kernel, element-wise energies
// ---------------------------------------------------------------------------------
struct ChainArgs {
  float* x;
  int64_t n_elem;
  int32_t dim;
  int32_t k_steps;
  StepCoef c;
  const float4* table;  // [k] or null
  int clamp_on;
  float cmin, cmax;
  int32_t thin;
  int32_t n_kept;
  float* traj;
  const float* noise;  // [k][n_elem] or null
  float s0, s1;
  RngKey key;
  uint64_t step0;
  diag::DiagArgs diag;  // per-block diagnostics records at the kept steps (DIAG kernels)
  float fold_eta;       // E = 2^m * eta, 2^m = 4 * s0: the drift coefficient of the folded DoubleWell loop (lean_fold_ok)
  const float* src;     // the start state, read once in the prologue; == x unless the call came through ebm_langevin_chain_from_f32
};

// everything but `noise` and `diag`, which the two launchers set apart
inline ChainArgs elem_chain_args(const LangevinChainReq& q) {
  ChainArgs a{};
  a.x = q.x; a.src = q.src; a.n_elem = q.n_chains * (int64_t)q.dim; a.dim = q.dim; a.k_steps = q.k_steps;
  a.c = StepCoef{q.eta, q.sqrt_eta, q.noise_coef};
  a.table = reinterpret_cast<const float4*>(q.coef_table);
  a.clamp_on = q.clamp; a.cmin = q.cmin; a.cmax = q.cmax;
  a.thin = q.thin; a.n_kept = q.n_kept(); a.traj = q.traj;
  a.s0 = q.e.s[0]; a.s1 = q.e.s[1];
  a.key = q.key(); a.step0 = q.offset;
  return a;
}

extern __shared__ __attribute__((aligned(16))) float elem_smem[];

// ---------------------------------------------------------------------------------
// Lean variant (native RNG): nothing but Philox + Box-Muller + gradient + update
// inside the loop.  The per-step coefficient table (schedulers, the Energy-Matching temperature
// sweep), the clamp and the thinned trajectory store are compile-time switches, so the headline case -- constant coefficients,
// no clamp -- carries neither a branch nor a live register for them.  One float4 group per lane:
// 2 or 4 independent groups per lane were measured and change nothing (8.96 / 9.05 / 8.91 ms on
// config 2; the loop is VALU-issue bound at 8 waves/SIMD either way).
// ---------------------------------------------------------------------------------
// DIAG: at every kept step the workgroup also reduces its 1024 elements to one diagnostics record (diag.h):
// the block's column sums / M2 and its energy sum are stored -- the population statistics of
// return_diagnostics=True without leaving the k-step launch.  Lanes past the end of the state stay in the
// loop (they take part in the workgroup barriers) with nothing to load or store.  The k steps are then walked
// as n_kept runs of `thin` steps (the hot inner loop is the plain one, unrolled by two).
// CONTRACT (ABI 8, EBM_CHAIN_CONTRACTED; the opt-in of `sampler.fused_arithmetic = True` on LangevinDynamics): the same step with the arithmetic
// contracted -- the gradient's x^2 - b^2 and the drift x - eta g as fused multiply-adds, the noise coefficient folded into the
// Box-Muller radius (ebm_common.h scaled_normal4_of): 6 of the loop's 72 vector instructions per float4 group and step fewer
// (66 against 72; both at 32-bit Philox counters).  NOT the
// reference's rounding (eager torch rounds every multiply and add); the same law, moments and Philox field.
// C64: the Philox counter at its full width, (group lo, group hi, step lo, step hi).  Otherwise (lean_counters32) both high
// words are 0 for the whole launch and the draw is ebm_common.h's PhiloxLane32: the same numbers, two vector multiplies and
// four logic ops fewer per float4 group and step (76 -> 72 vector instructions on the plain DoubleWell loop).
//
// FOLD (KIND == kDoubleWellFold, the plain DoubleWell call when lean_fold_ok holds): the gradient's power-of-two factor
// 2^m = 4 h moves into the drift coefficient, E = 2^m eta (exact, computed on the host).  Per pair of elements
//   v = fl(fl(fl(x x) - b^2) x),   x1 = fl(x - fl(E v))
// where the literal loop computes g = fl(fl(2^m u) x), x1 = fl(x - fl(eta g)): one packed multiply fewer per pair, 72 -> 70
// vector instructions per float4 group and step.  The noise chain is unchanged.  Why the two agree bit for bit (u = fl(x x) - b^2,
// b^2 = 1, m >= 0, eta >= 2^-60, |noise_coef sqrt_eta| <= 2^60):
//  * fl(2^m u) = 2^m u exactly unless it overflows; then the literal g is +-inf, and either u x overflows too (both forms give
//    the same +-inf; at m = 3 this needs |x| > 2^62) or 2^m v does: the window below.
//  * Otherwise fl(2^m u x) = 2^m fl(u x) = 2^m v whenever v is normal and 2^m v is finite (rounding commutes with a power-of-two
//    scale in the normal range), and fl(eta 2^m v) = fl(E v): the same real product rounded once.  Signed zeros agree.
//  * v is subnormal only for |x| < 2^-102: u is 0 or |u| >= 2^-24 (Sterbenz near |x| = 1), and for tiny x, u = -1 exactly, so
//    v = -x exactly and g = -2^m x exactly.  Non-finite x gives the same inf / NaN in both forms.
//  * They differ only in the overflow window FLT_MAX / 2^m < |v| <= FLT_MAX (|x| ~ 3.5e12 at m = 3): the literal g is +-inf,
//    the folded |E v| >= eta 2^127 >= 2^67 (or +-inf, which agrees).  The window absorbs: |x| <= 2^43 there and the noise term is below
//    2^63 (Box-Muller radius <= 6.8), so the next state has |x| >= 2^66, then x x overflows and the state is +-inf, then NaN.
// Hence a lane whose four final values are finite with |x| < 2^60 never entered the window and equals the literal loop bit for
// bit.  Every other lane runs the literal loop again from its start values (kept in registers) over all k steps -- after the
// step loop, so the guard costs the loop nothing.
//
// PLAIN (KIND == kDoubleWellFoldPlain, langevin_fold.hip: what the launcher takes whenever the fold applies): the folded step with
// gradient, drift and noise update written one element at a time, compiled with -fno-slp-vectorize so they stay v_mul_f32 /
// v_sub_f32 / v_add_f32 -- the same IEEE operations in the same order, so the same bits.  88 vector instructions per float4 group
// and step where the 2-vector form issues 70 (its 16 v_pk_mul_f32 / v_pk_add_f32 and the two the vectoriser packs in Box-Muller
// as 36 plain ones), and 1.1 - 1.3 % faster: in this loop a packed-f32 instruction takes more issue time than two plain ones
// (docs/design/langevin_flat.md; going the other way, packing Box-Muller's prep as well, 67 instructions, is 0.8 % slower).
template <int KIND, bool TABLE, bool CLAMP, bool TRAJ, bool HEUN, bool DIAG, bool CONTRACT, bool C64>
__device__ __forceinline__ void lean_body(const ChainArgs& a) {
  constexpr bool PLAIN = KIND == kDoubleWellFoldPlain;
  constexpr bool FOLD = KIND == kDoubleWellFold || PLAIN;
  constexpr bool DW = KIND == EBM_ENERGY_DOUBLE_WELL || FOLD;  // the arithmetic of the literal steps
  static_assert(!FOLD || (!TABLE && !CLAMP && !TRAJ && !HEUN && !DIAG && !CONTRACT), "the fold exists for the plain lean call only");
  const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t e0 = g * 4;
  if constexpr (!DIAG) {
    if (e0 >= a.n_elem) return;
  }
  const int64_t left = a.n_elem - e0;
  const int nv = left >= 4 ? 4 : (left > 0 ? (int)left : 0);
  F4 x = load4(a.src, e0 < a.n_elem ? e0 : 0, nv, true);
  StepCoef c = a.c;
  // lanes past the end of the state (DIAG only) draw from a truncated counter and store nothing
  const PhiloxLane32 rng((uint32_t)g, a.key);
  const uint32_t step0 = (uint32_t)a.step0;
  auto draw = [&](int i) -> U4 {
    if constexpr (C64) return philox_at(a.key, (uint64_t)g, a.step0 + (uint64_t)i);
    else return rng.at(step0 + (uint32_t)i);
  };
  // TRAJ (dim % 4 == 0 only, so a lane's float4 never straddles two chains): traj[c, j, d..d+3]
  float* tptr = nullptr;
  if constexpr (TRAJ) {
    const int64_t chain = e0 / a.dim;
    tptr = a.traj + chain * (int64_t)a.n_kept * a.dim + (e0 - chain * a.dim);
  }
  auto one_step = [&](int i) {
    if constexpr (TABLE) {  // wave-uniform: scalar loads
      const float4 t = a.table[i];
      c.eta = t.x; c.sqrt_eta = t.y; c.noise_coef = t.z;
    }
    if constexpr (CONTRACT) {
      static_assert(!TABLE && !CLAMP && !HEUN, "the contracted form exists for the plain call only");
      const F4 e = scaled_normal4_of(draw(i), c.noise_coef * c.sqrt_eta);  // (uniform product: scalar unit)
#pragma unroll
      for (int q = 0; q < 4; q += 2) {
        const v2f xv = {x.v[q], x.v[q + 1]}, ev = {e.v[q], e.v[q + 1]};
        v2f gr;
        if constexpr (KIND == EBM_ENERGY_DOUBLE_WELL) gr = ((4.0f * a.s0) * __builtin_elementwise_fma(xv, xv, v2f{-a.s1, -a.s1})) * xv;
        else gr = (2.0f * a.s0) * xv;
        const v2f nv2 = __builtin_elementwise_fma(v2f{-c.eta, -c.eta}, gr, xv) + ev;
        x.v[q] = nv2.x;
        x.v[q + 1] = nv2.y;
      }
      return;
    }
    const F4 eps = normal4_of(draw(i));
    // gradient + update on explicit 2-vectors (packed-f32 instructions); written out this way because
    // the clamp's min/max would otherwise make the compiler fall back to scalar arithmetic for all of it
#pragma unroll
    for (int q = 0; q < 4; q += 2) {
      const v2f xv = {x.v[q], x.v[q + 1]}, ev = {eps.v[q], eps.v[q + 1]};
      v2f gr;
      if constexpr (DW) gr = ((4.0f * a.s0) * (xv * xv - a.s1)) * xv;  // see elem_grad
      else gr = (2.0f * a.s0) * xv;
      if constexpr (HEUN) {  // predictor x - eta*g0, corrector gradient 0.5*g0 + 0.5*g(predictor)
        const v2f xp = xv - c.eta * gr;
        v2f g1;
        if constexpr (KIND == EBM_ENERGY_DOUBLE_WELL) g1 = ((4.0f * a.s0) * (xp * xp - a.s1)) * xp;
        else g1 = (2.0f * a.s0) * xp;
        gr = 0.5f * gr + 0.5f * g1;
      }
      const v2f x1 = xv - c.eta * gr;
      const v2f dw = ev * c.sqrt_eta;
      v2f nv2 = x1 + c.noise_coef * dw;
      if constexpr (CLAMP) nv2 = __builtin_elementwise_minimum(__builtin_elementwise_maximum(nv2, v2f{a.cmin, a.cmin}), v2f{a.cmax, a.cmax});
      x.v[q] = nv2.x;
      x.v[q + 1] = nv2.y;
    }
  };
  if constexpr (FOLD) {
    const F4 x_start = x;
    auto fold_step = [&](int i) {
      const F4 eps = normal4_of(draw(i));
      if constexpr (PLAIN) {  // the same operations, one element each
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float xs = x.v[q];
          const float v = (xs * xs - a.s1) * xs;
          const float x1 = xs - a.fold_eta * v;
          const float dw = eps.v[q] * c.sqrt_eta;
          x.v[q] = x1 + c.noise_coef * dw;
        }
        return;
      }
#pragma unroll
      for (int q = 0; q < 4; q += 2) {
        const v2f xv = {x.v[q], x.v[q + 1]}, ev = {eps.v[q], eps.v[q + 1]};
        const v2f v = (xv * xv - a.s1) * xv;  // fl(u x): the gradient is 2^m v
        const v2f x1 = xv - a.fold_eta * v;   // fl(E v) == fl(eta g) outside the overflow window
        const v2f dw = ev * c.sqrt_eta;
        const v2f nv2 = x1 + c.noise_coef * dw;
        x.v[q] = nv2.x;
        x.v[q + 1] = nv2.y;
      }
    };
#pragma unroll 2  // as the literal loop
    for (int i = 0; i < a.k_steps; ++i) fold_step(i);
    // NaN fails every comparison: one test covers non-finite values and the window's aftermath
    const bool clean = (__builtin_fabsf(x.v[0]) < 0x1p60f) & (__builtin_fabsf(x.v[1]) < 0x1p60f) &
                       (__builtin_fabsf(x.v[2]) < 0x1p60f) & (__builtin_fabsf(x.v[3]) < 0x1p60f);
    if (!clean) {  // the literal loop from the start values, for these lanes only
      x = x_start;
#pragma unroll 1
      for (int i = 0; i < a.k_steps; ++i) one_step(i);
    }
  } else if constexpr (!DIAG) {
    int until_keep = a.thin;
#pragma unroll 2  // measured: 9.00 -> 8.83 ms on config 2 (4 gives no more)
    for (int i = 0; i < a.k_steps; ++i) {
      one_step(i);
      if constexpr (TRAJ) {
        if (--until_keep == 0) {  // wave-uniform
          until_keep = a.thin;
          *reinterpret_cast<float4*>(tptr) = make_float4(x.v[0], x.v[1], x.v[2], x.v[3]);
          tptr += a.dim;
        }
      }
    }
  } else {
    const int64_t block_e0 = (int64_t)blockIdx.x * (kBlock * 4);
    const int64_t rest = a.n_elem - block_e0;
    const int L = rest >= kBlock * 4 ? kBlock * 4 : (int)rest;  // valid elements of this workgroup
    const bool fast = diag::fast_flat_ok(a.dim);
    const int rows_b = L / a.dim;
    const float inv_rows = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(rows_b > 0 ? 1.0f / (float)rows_b : 0.0f)));
    int i = 0;
    for (int keep = 0; keep < a.n_kept; ++keep) {
      const int stop = i + a.thin;
#pragma unroll 2
      for (; i < stop; ++i) one_step(i);
      if constexpr (TRAJ) {
        if (nv == 4) *reinterpret_cast<float4*>(tptr) = make_float4(x.v[0], x.v[1], x.v[2], x.v[3]);
        tptr += a.dim;
      }
      float e_part = 0.0f;  // sum over the lane's elements of the per-coordinate energy term
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float t;
        if constexpr (KIND == EBM_ENERGY_DOUBLE_WELL) { const float u = x.v[q] * x.v[q] - a.s1; t = u * u; }
        else t = x.v[q] * x.v[q];
        e_part += (q < nv) ? t : 0.0f;
      }
      if (fast) {
        diag::emit_flat_fast(a.diag, keep, elem_smem, a.dim, make_float4(x.v[0], x.v[1], x.v[2], x.v[3]), L, inv_rows, a.s0 * e_part);
      } else {
        *reinterpret_cast<float4*>(elem_smem + 4 * threadIdx.x) = make_float4(x.v[0], x.v[1], x.v[2], x.v[3]);
        diag::emit(a.diag, keep, elem_smem, elem_smem + a.diag.E, L, a.dim, a.s0 * e_part, 0.0f);
      }
    }
#pragma unroll 2
    for (; i < a.k_steps; ++i) one_step(i);  // the trailing k % thin steps
  }
  if (nv > 0) store4(a.x, e0, nv, true, x);
}

template <int KIND, bool TABLE, bool CLAMP, bool TRAJ, bool HEUN, bool C64>
__global__ __launch_bounds__(kBlock) void langevin_chain_lean_kernel(ChainArgs a) {
  lean_body<KIND, TABLE, CLAMP, TRAJ, HEUN, false, false, C64>(a);
}
template <int KIND, bool C64>
__global__ __launch_bounds__(kBlock) void langevin_chain_lean_contracted_kernel(ChainArgs a) {
  lean_body<KIND, false, false, false, false, false, true, C64>(a);
}

// The DIAG form, held to 64 VGPRs (8 waves per SIMD like the plain kernel: the out-of-line generic emit() would
// otherwise set the kernel's register count to 80 and cost the step loop 4 %).  A template-dependent expression in
// __launch_bounds__ is ignored by hipcc 7.2, hence the second entry point.
template <int KIND, bool TABLE, bool CLAMP, bool TRAJ, bool HEUN, bool C64>
__global__ __launch_bounds__(kBlock, 8) void langevin_chain_lean_diag_kernel(ChainArgs a) {
  lean_body<KIND, TABLE, CLAMP, TRAJ, HEUN, true, false, C64>(a);
}

// The lean kernels take the 32-bit counter words (C64 = false) when every lane's group index and every step of the launch fit
// 32 bits: ceil(n_elem / 4) <= 2^32 and step0 + k_steps <= 2^32 (no carry into the step's high word).  Larger states and
// generator offsets run the C64 instantiations, whose draws are the same function of the full counter.
inline bool lean_counters32(const ChainArgs& a) {
  const uint64_t two32 = 1ull << 32;
  const uint64_t k = a.k_steps > 0 ? (uint64_t)a.k_steps : 0;
  return (uint64_t)ceil_div64(a.n_elem, 4) <= two32 && a.step0 <= two32 - k;
}

// The folded DoubleWell loop's preconditions on the call's constants (lean_body FOLD): 4 s0 = 2^m with m >= 0, b^2 == 1,
// eta >= 2^-60 with E = 2^m eta finite, |noise_coef sqrt_eta| <= 2^60.  Sets a.fold_eta = E (ldexp: exact).  The caller checks
// the rest: DoubleWell, the plain lean call (no table, clamp, trajectory, Heun, injected noise or records).
inline bool lean_fold_ok(ChainArgs& a) {
  int e2 = 0;
  const float four_h = 4.0f * a.s0;  // the literal loop's factor
  if (!std::isfinite(four_h) || std::frexp(four_h, &e2) != 0.5f || e2 < 1) return false;  // four_h = 2^(e2 - 1)
  if (a.s1 != 1.0f || !(a.c.eta >= 0x1p-60f)) return false;
  const float E = std::ldexp(a.c.eta, e2 - 1);
  if (!std::isfinite(E) || !(std::fabs((double)a.c.noise_coef * (double)a.c.sqrt_eta) <= 0x1p60)) return false;
  a.fold_eta = E;
  return true;
}

}  // namespace
}  // namespace ebm
