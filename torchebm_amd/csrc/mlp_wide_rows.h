// What the walks on the wide MLP energy share besides the evaluation (docs/design/mlp_wide.md, "Shared code of the walks"):
// the lane-layout helpers -- rows of a [.., dim] matrix to and from the 32x32 C/D layout, the normal field a register quad at a
// time, the plain kinetic energy --, the blocks of the step loops that are shared as text (macros), the running moments, the
// macros that go with the plain evaluation (mlp_wide_plain_eval.inc) and the host launcher.  Users: the bodies of the nine walks,
// mlp_wide_{hmc,ais,kinetic,ghmc,tempering,kinetic_moments,ghmc_moments,langevin_moments,tempering_langevin}_body.h; the leapfrog
// state machine of the AIS, GHMC and tempered-HMC walks is text of its own, mlp_wide_leapfrog.inc.  How a helper is spelled and
// called decides registers and schedule of kernels at the register limit; where a body keeps a block in its own words, it says
// what the helper cost.
#pragma once
#include <type_traits>
#include "mlp_wide_body.h"

namespace ebm {
namespace widemlp {

// The lane geometry of mlp_wide_setup.inc and the lane's K-half, all four by REFERENCE to the kernel's own variables
// (EBM_WIDE_LANES() behind the set-up).  This is not a neutral spelling.  Measured on the kinetic H = 64 unit: by reference the
// four kernels are the hand-inlined lambdas' instruction for instruction; with dim / quads / active copied into the struct three
// of them take 8, 3 and 2 more VGPRs; with the K-half passed to the helpers by value three of them come out with another
// schedule (62 460 -> 62 869 lines of disassembly).  A walk that keeps an opaque copy of its K-half inside its step loop
// (EBM_WIDE_STEP_COPIES_OPAQUE below) binds a second Lanes to that copy there.
struct Lanes {
  const int& dim;
  const bool& quads;   // a register quad r = 4q .. 4q+3 is four consecutive, 16-byte aligned columns
  const bool& active;  // the lane's chain exists
  const int& h;        // the lane's K-half
};
#define EBM_WIDE_LANES() const Lanes lanes{dim, quads, active, h}

// rows of a [.., dim] matrix into the C/D layout, zero beyond dim and for the lanes past the last chain
template <int DT>
__device__ __forceinline__ void load_rows(const Lanes& L, float (&dst)[DT][16], const float* src, int64_t row) {
  const int hq = L.h;
#pragma unroll
  for (int td = 0; td < DT; ++td)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c0 = 32 * td + 8 * q + 4 * hq;
      if (L.quads && L.active && c0 + 3 < L.dim) {
        const float4 w = *reinterpret_cast<const float4*>(src + row * L.dim + c0);
        dst[td][4 * q] = w.x; dst[td][4 * q + 1] = w.y; dst[td][4 * q + 2] = w.z; dst[td][4 * q + 3] = w.w;
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) dst[td][4 * q + i] = (L.active && c0 + i < L.dim) ? src[row * L.dim + c0 + i] : 0.0f;
      }
    }
}

// ... and back (callers guard with `active`; columns past dim never reach memory)
template <int DT>
__device__ __forceinline__ void store_rows(const Lanes& L, float* dst, int64_t row, const float (&src)[DT][16]) {
  const int hq = L.h;
#pragma unroll
  for (int td = 0; td < DT; ++td)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = 32 * td + row_of(r, hq);
      if (c < L.dim) dst[row * L.dim + c] = src[td][r];
    }
}

// one register quad of the normal field at `step`, element chain * dim + col (zero beyond dim): one Philox counter where a
// quad is four aligned columns, per element otherwise
__device__ __forceinline__ void normal_quad(const Lanes& L, float (&z)[4], RngKey key, int c0, int64_t row, uint64_t step) {
#pragma unroll
  for (int i = 0; i < 4; ++i) z[i] = 0.0f;
  if (c0 < L.dim) {
    if (L.quads) {
      const F4 nrm = normal4_at(key, ((uint64_t)row * (uint64_t)L.dim + (uint64_t)c0) >> 2, step);
#pragma unroll
      for (int i = 0; i < 4; ++i) z[i] = nrm.v[i];
    } else {
      uint64_t have = ~0ull;
      F4 nrm;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint64_t e = (uint64_t)row * (uint64_t)L.dim + (uint64_t)(c0 + i);
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
  for (int i = 0; i < 4; ++i) z[i] = (c0 + i < L.dim) ? z[i] : 0.0f;
}

// ---- Blocks of the walks' step loops, shared as TEXT.  The walk kernels sit at the register limit, and a block of theirs put
// into a function -- __forceinline__, a lambda, a by-value return, a callable -- comes out as other code: the noise quad below
// changed every BAOAB kernel (62 460 -> ~65 000 lines of disassembly, up to 22 more VGPRs) and the register counts of every GHMC
// kernel, the swap decision both tempered units.  As a macro the block is the tokens the body used to spell out, and every kernel
// is the instructions it was (docs/design/mlp_wide.md, "Shared code of the walks").  The macros read the names of the set-up
// and of the loop they stand in (named at each) and declare the ones they say.

// In front of every evaluation of a step loop: opaque per-iteration copies smp / hq / key of the chain index, the lane's K-half
// and the key.  Nothing derived from them is then hoisted out of the loop and spilled around every evaluation: left invariant,
// the 64-bit column offsets of the Philox counters (a register pair per element), the column masks (a scalar pair each) and the
// round keys are all formed in front of the loop and live through it (docs/design/kinetic_mlp.md).  The helpers above see the
// opaque K-half through a second Lanes bound to hq.
#define EBM_WIDE_STEP_COPIES_OPAQUE() \
  int64_t smp = sample;               \
  int hq = h;                         \
  RngKey key = a.key;                 \
  asm volatile("" : "+v"(smp), "+v"(hq), "+s"(key.k0), "+s"(key.k1))

// float Z[4]: the step's noise of the register quad at column c0, injected (NOISE, the step's [n_chains, dim] plane, or null)
// or drawn at Philox step STEP through the Lanes L.  Reads quads, active, dim, c0, smp, key.
#define EBM_WIDE_NOISE_QUAD(Z, NOISE, L, STEP)                                                                         \
  float Z[4];                                                                                                          \
  if (NOISE) {                                                                                                         \
    if (quads && active && c0 + 3 < dim) {                                                                             \
      const float4 w = *reinterpret_cast<const float4*>(NOISE + smp * dim + c0);                                       \
      Z[0] = w.x; Z[1] = w.y; Z[2] = w.z; Z[3] = w.w;                                                                  \
    } else {                                                                                                           \
      _Pragma("unroll") for (int j = 0; j < 4; ++j) Z[j] = (active && c0 + j < dim) ? NOISE[smp * dim + c0 + j] : 0.0f; \
    }                                                                                                                  \
  } else {                                                                                                             \
    normal_quad(L, Z, key, c0, smp, STEP);                                                                             \
  }

// The Euler-Maruyama update of the quad (td, q) at c0:  x1 = x - eta g;  dw = z sqrt_eta;  x' = x1 + noise_coef dw, every
// operation rounded on its own.  Reads td, q, c0, xr, g, z, eta, sqrt_eta, noise_coef, dim.
#define EBM_WIDE_EULER_MARUYAMA_QUAD()                \
  _Pragma("unroll") for (int j = 0; j < 4; ++j) {     \
    const int r = 4 * q + j;                          \
    const float x1 = xr[td][r] - eta * g[td][r];      \
    const float dw = z[j] * sqrt_eta;                 \
    const float nv = x1 + noise_coef * dw;            \
    xr[td][r] = (c0 + j < dim) ? nv : 0.0f;           \
  }

// The swap event of the tempered walks, decided: slot s pairs with s + 1 when s has the event's parity, with s - 1 otherwise
// (the ends may be unpaired); both partners -- neighbouring lanes of one K-half -- form the same delta from the same two energies
// and read the same uniform, the lower slot's: U, the caller's [n_events, n_chains] or null, else the draw at Philox step STEP.
// E_NOW is the energy of the state the lane's slot holds.  Declares parity, lower, lo, paired, partner and swap; reads slot,
// event, R, lane, active, smp, key, a.beta, a.n_chains.
#define EBM_WIDE_SWAP_DECISION(E_NOW, U, STEP)                                                                          \
  const int parity = event & 1;                                                                                        \
  const bool lower = ((slot - parity) & 1) == 0;                                                                       \
  const int lo = lower ? slot : slot - 1;                                                                              \
  const bool paired = active && lo >= parity && lo + 1 < R;                                                            \
  const int partner = paired ? (lower ? lane + 1 : lane - 1) : lane;                                                   \
  const float e_other = __shfl(E_NOW, partner);                                                                        \
  bool swap = false;                                                                                                   \
  if (paired) {                                                                                                        \
    const float e_lo = lower ? E_NOW : e_other, e_hi = lower ? e_other : E_NOW;                                        \
    const float delta = (a.beta[lo] - a.beta[lo + 1]) * (e_lo - e_hi);                                                 \
    const int64_t urow = lower ? smp : smp - 1;                                                                        \
    float us;                                                                                                          \
    if (U) us = U[(int64_t)event * a.n_chains + urow];                                                                 \
    else us = u01_half_open(pick(philox_at(key, (uint64_t)urow >> 2, STEP), (int)(urow & 3)));                         \
    swap = delta == delta && us < expf(fminf(delta, 0.0f));                                                            \
  }

// The Welford bookkeeping of the counted state J (0-based behind the burn-in) of a running-moments walk: which half it falls in,
// c (c + 1 states of this half with this one), rc = float32(1 / (c + 1)) by a wave-uniform load, and first: the pair starts from
// zero.  Reads a.half_len, a.recip.
#define EBM_WIDE_MOMENTS_COUNT(J)               \
  const bool second = (J) >= a.half_len;        \
  const int c = second ? (J) - a.half_len : (J); \
  const float rc = a.recip[c];                  \
  const bool first = c == 0
// ... and float* NAME, the half's planes of BASE (the second half lies STRIDE floats behind the first), through an opaque copy
// of the pointer: nothing of a plane is forwarded from one counted step to the next in registers
#define EBM_WIDE_MOMENTS_PLANES(NAME, BASE, STRIDE) \
  float* NAME = BASE + (second ? STRIDE : 0);       \
  asm volatile("" : "+s"(NAME))

// The running moments of a walk kept in the CALLER's planes (mlp_wide_kinetic_moments_body.h, mlp_wide_ghmc_moments_body.h;
// docs/design/kinetic_moments_mlp.md): one in-place update of a row, a register quad at a time, so nothing of a plane lives in
// registers through an evaluation.  A lane reads back only what it stored itself (the columns of load_rows / store_rows);
// `first` (wave-uniform): the pair starts from zero and the planes are NOT read.  Every operation is rounded on its own (the
// units compile with -ffp-contract=off).  VSQ == false, the Welford pair of q with rc = recip[c - 1]:
//     d = q - mean;   mean = mean + d * rc;   M2 = M2 + d * (q - mean)
// VSQ == true, the running mean of q^2 (m2 is not touched):   m = m + (q * q - m) * rc
template <bool VSQ, int DT>
__device__ __forceinline__ void moments_rows(const Lanes& L, float* mean, float* m2, int64_t row, const float (&q)[DT][16], float rc,
                                             bool first) {
  if (!L.active) return;
  const int hq = L.h;
#pragma unroll
  for (int td = 0; td < DT; ++td)
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
      const int c0 = 32 * td + 8 * qd + 4 * hq;
      float* const pm = mean + row * L.dim + c0;
      float* const ps = m2 + row * L.dim + c0;
      const bool whole = L.quads && c0 + 3 < L.dim;
      float mu[4] = {0.0f, 0.0f, 0.0f, 0.0f}, s2[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      if (!first) {
        if (whole) {
          const float4 w = *reinterpret_cast<const float4*>(pm);
          mu[0] = w.x; mu[1] = w.y; mu[2] = w.z; mu[3] = w.w;
          if constexpr (!VSQ) {
            const float4 y = *reinterpret_cast<const float4*>(ps);
            s2[0] = y.x; s2[1] = y.y; s2[2] = y.z; s2[3] = y.w;
          }
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (c0 + i < L.dim) {
              mu[i] = pm[i];
              if constexpr (!VSQ) s2[i] = ps[i];
            }
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float qi = q[td][4 * qd + i];
        if constexpr (VSQ) {
          const float vv = qi * qi;
          mu[i] = mu[i] + (vv - mu[i]) * rc;
        } else {
          const float d = qi - mu[i];
          mu[i] = mu[i] + d * rc;
          s2[i] = s2[i] + d * (qi - mu[i]);
        }
      }
      if (whole) {
        *reinterpret_cast<float4*>(pm) = make_float4(mu[0], mu[1], mu[2], mu[3]);
        if constexpr (!VSQ) *reinterpret_cast<float4*>(ps) = make_float4(s2[0], s2[1], s2[2], s2[3]);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (c0 + i < L.dim) {
            pm[i] = mu[i];
            if constexpr (!VSQ) ps[i] = s2[i];
          }
      }
    }
}
// ... and of one number per chain (the energy), by the lane of K-half 0
__device__ __forceinline__ void moments_scalar(const Lanes& L, float* mean, float* m2, int64_t row, float e, float rc, bool first) {
  if (!L.active || L.h != 0) return;
  float mu = 0.0f, s2 = 0.0f;
  if (!first) {
    mu = mean[row];
    s2 = m2[row];
  }
  const float d = e - mu;
  mu = mu + d * rc;
  s2 = s2 + d * (e - mu);
  mean[row] = mu;
  m2[row] = s2;
}

// sum q^2 over the whole chain (both K-halves; the padding registers are zero)
template <int DT>
__device__ __forceinline__ float sum_squares(const float (&q)[DT][16]) {
  float acc = 0.0f;
#pragma unroll
  for (int td = 0; td < DT; ++td)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc += q[td][r] * q[td][r];
  acc += __shfl_xor(acc, 32);
  return acc;
}
// 0.5 p^T p, clamped to [0, 1e10]
template <int DT>
__device__ __forceinline__ float kinetic_plain(const float (&q)[DT][16]) {
  return clamp_nanprop(0.5f * sum_squares<DT>(q), 0.0f, 1e10f);
}

// The plain evaluation (mlp_wide_plain_eval.inc) reads the images through walk1_once / walk2_once.  Behind the set-up a walk
// says which they are.  OPAQUE: the images' LDS addresses formed once, an opaque scalar each -- left visible, the conversion of
// the LDS pointer is re-derived at its uses inside the evaluation when registers run out (first met in the AIS kernel at H = 128
// and two state tiles), in a form the backend rejects.  SETUPS: the set-up's own walks under that name, for the HMC kernels,
// which were tuned without the trick and keep their code.
#define EBM_WIDE_WALKS_ONCE_OPAQUE() \
  auto walk1_once = walk1;           \
  auto walk2_once = walk2;           \
  asm volatile("" : "+s"(walk1_once.base), "+s"(walk2_once.base))
#define EBM_WIDE_WALKS_ONCE_SETUPS() \
  const auto& walk1_once = walk1;    \
  const auto& walk2_once = walk2

// One launch of KERNEL, an instantiation of a walk kernel at (HT, DT, MODE) that takes Args by value: the per-device LDS opt-in,
// one wave per 32 chains, the launch.
template <auto KERNEL, int HT, int DT, int MODE, class Args>
int launch_walk(const Args& a, hipStream_t st, const char* who) {
  const size_t smem = wide_smem_bytes(HT, DT, MODE);
  static DeviceOnce attr_once;  // the LDS opt-in is a per-device function attribute
  if (attr_once.first()) {  // > 64 KiB of dynamic LDS needs the opt-in
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  }
  const int64_t blocks = ceil_div64(a.n_chains, 32 * (kBlock / 64));
  if (blocks > 0x7fffffffLL) return fail(EBM_EINVAL, "%s: too many chains for one launch", who);
  hipLaunchKernelGGL(KERNEL, dim3((unsigned)blocks), dim3(kBlock), smem, st, a);
  return check_launch(who);
}

// ... of the kernel for a.dim among a family's at hidden width 32 HT, each at wide_mode(HT, DT).  WALK names the family:
//   template <int HT, int DT, int MODE> static constexpr auto kernel = &the_kernel<HT, DT, MODE>;
template <class WALK, int HT, class Args>
int launch_walk_by_dim(const Args& a, hipStream_t st, const char* who) {
  const auto at = [&](auto dt) {
    constexpr int DT = decltype(dt)::value, MODE = wide_mode(HT, DT);
    return launch_walk<WALK::template kernel<HT, DT, MODE>, HT, DT, MODE>(a, st, who);
  };
  switch ((a.dim + 31) / 32) {
    case 1: return at(std::integral_constant<int, 1>{});
    case 2: return at(std::integral_constant<int, 2>{});
    case 3: return at(std::integral_constant<int, 3>{});
    default: return at(std::integral_constant<int, 4>{});
  }
}

}  // namespace widemlp
}  // namespace ebm
