// The three test landscapes of the reference's core as lane-group energies (rows.h: Energy<KIND, LaneT>):
// Rosenbrock (base_model.py:232-264), Ackley (:267-294), Rastrigin (:297-316).  Scalars only, no LDS.
// A header of its own, included after rows.h by the units that instantiate these kinds (rows_langevin.hip and the per-kind
// units, *_unit.hip: one source serves every kind, so all its objects see this text and only the landscape kinds' objects
// instantiate it), so that every other unit compiles from the text it had.  docs/design/landscapes.md.
//
// The contract of rows.h holds here as there: slots with !L.ok(v, i) hold x = 0, must return g = 0 and add nothing to
// the energy.  It bites three times: cos(0) = 1 (a padded slot would add -a to Rastrigin's sum and 1 to Ackley's mean
// cosine), the mean is over dim, not over the padded width, and column dim would be read as x_{i+1} of a Rosenbrock
// term i = dim - 1 that does not exist.
#pragma once
#include "rows.h"

namespace ebm {
namespace rows {

// sin / cos of c x.  c == 2 pi (Rastrigin always, Ackley's default): sinpi / cospi of 2 x -- the doubling is exact, there
// is no argument product to round and no range reduction (about 60 instructions against 160 for sincosf with its
// large-argument path).  Any other c: sin / cos of the fp32 product, what the reference's fp32 ops compute.
__device__ __forceinline__ void sincos_2pi_x(float xv, float& s, float& co) { sincospif(2.0f * xv, &s, &co); }
template <bool TWO_PI>
__device__ __forceinline__ void sincos_cx(float c, float xv, float& s, float& co) {
  if constexpr (TWO_PI) sincos_2pi_x(xv, s, co);
  else sincosf(c * xv, &s, &co);
}

// Neighbour exchange along a chain row.  In the Lane layout vector v of lane lg holds columns (v G + lg) 4 .. + 3, so the
// vector that FOLLOWS it in the row is vector v of lane lg + 1 -- or vector v + 1 of lane 0 when lg is the group's last lane.
//   from_next<G>(same, wrap, lg): lane lg + 1's `same`; the last lane of the group gets lane 0's `wrap`
//   from_prev<G>(same, wrap, lg): lane lg - 1's `same`; lane 0 gets the last lane's `wrap`
// Up to 16 lanes a group lies inside one DPP row: row_shl:1 / row_shr:1 for the neighbour, row_shr:(G-1) / row_shl:(G-1)
// for the wrap (bound_ctrl: a read past the row's end gives 0, and is never selected).  Groups of 32 / 64 lanes cross
// rows: one ds_bpermute of a rotation, each source lane publishing what its reader wants.  No lane ever reads another
// group, so the neighbouring chain cannot leak in.
template <int G>
__device__ __forceinline__ float from_next(float same, float wrap, int lg) {
  if constexpr (G == 1) {
    return wrap;
  } else if constexpr (G <= 16) {
    const float a = dpp_f<0x101>(same);          // row_shl:1: lane i reads lane i + 1
    const float b = dpp_f<0x110 + (G - 1)>(wrap);  // row_shr:(G-1): lane i reads lane i - (G - 1)
    return lg == G - 1 ? b : a;
  } else {
    const int lane = threadIdx.x & 63;
    const float pub = lg == 0 ? wrap : same;
    return __shfl(pub, (lane & ~(G - 1)) | ((lane + 1) & (G - 1)));
  }
}
template <int G>
__device__ __forceinline__ float from_prev(float same, float wrap, int lg) {
  if constexpr (G == 1) {
    return wrap;
  } else if constexpr (G <= 16) {
    const float a = dpp_f<0x111>(same);          // row_shr:1: lane i reads lane i - 1
    const float b = dpp_f<0x100 + (G - 1)>(wrap);  // row_shl:(G-1): lane i reads lane i + (G - 1)
    return lg == 0 ? b : a;
  } else {
    const int lane = threadIdx.x & 63;
    const float pub = lg == G - 1 ? wrap : same;
    return __shfl(pub, (lane & ~(G - 1)) | ((lane + G - 1) & (G - 1)));
  }
}

// ---------------------------------------------------------------------------------
// Rastrigin:  E = a n + sum_j x_j^2 - a cos(2 pi x_j),   g_j = 2 x_j + 2 pi a sin(2 pi x_j).
// Element-wise plus one group_sum.  The energy is summed as x^2 + a (1 - cos): every term is >= 0 (no a n - a n
// cancellation at the bottom of a well) and n never enters, so the padded width cannot.
// Finite E => x finite (x^2 is a term) and g finite: no check value needed.
// ---------------------------------------------------------------------------------
template <class LaneT>
struct Energy<EBM_ENERGY_RASTRIGIN, LaneT> {
  static constexpr int G = LaneT::G, NV = LaneT::NV;
  static constexpr bool HAS_GRAD_ONLY = false;
  float a, k;  // k = 2 pi a
  __device__ __forceinline__ void init(const EnergyParams& P, const LaneT&, const Smem&) {
    a = P.s0;
    k = 6.283185307179586f * P.s0;
  }
  template <bool WANT_E>
  __device__ __forceinline__ float eval(const LaneT& L, const Slice<NV>& x, Slice<NV>& g) const {
    float acc = 0.0f;
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float xv = x.a[v][i];
        float s, co;
        sincos_2pi_x(xv, s, co);
        const bool ok = L.ok(v, i);
        g.a[v][i] = ok ? __builtin_fmaf(k, s, 2.0f * xv) : 0.0f;
        if (WANT_E) acc += ok ? __builtin_fmaf(a, 1.0f - co, xv * xv) : 0.0f;
      }
    if (!WANT_E) return 0.0f;
    return group_sum<G>(acc);
  }
};

// ---------------------------------------------------------------------------------
// Ackley:  E = -a exp(-b r) - exp(S2 / n) + a + e,   r = sqrt(S1 / n),  S1 = sum x^2,  S2 = sum cos(c x)
//          g_j = A x_j + B sin(c x_j),   A = a b exp(-b r) / (n r),   B = c exp(S2 / n) / n     (A, B group-uniform)
// Two group_sums per evaluation, with or without the energy.  At x = 0: r = 0, A = inf, g = inf * 0 = NaN in every
// coordinate -- what autograd returns there (the square root's backward), not repaired here.
// HMC check value.  E is finite for every finite x, also where the gradient is not: r == 0 (the origin, or squares that
// all underflow) makes A infinite.  That is the only such case: for r > 0 finite, A <= a b / (n r) and A |x_j| <= a b /
// sqrt(n) stay finite, B <= c e / n always; an infinite or NaN coordinate puts NaN into S2 (cos) and so into E.  So
// chk = E + 0 * A is finite exactly when E and every gradient component are.
// ---------------------------------------------------------------------------------
template <class LaneT>
struct Energy<EBM_ENERGY_ACKLEY, LaneT> {
  static constexpr int G = LaneT::G, NV = LaneT::NV;
  static constexpr bool HAS_GRAD_ONLY = false;
  static constexpr bool GRAD_CHECK = true;
  float a, b, c, n;
  bool two_pi;
  __device__ __forceinline__ void init(const EnergyParams& P, const LaneT& L, const Smem&) {
    a = P.s0; b = P.s1; c = P.s2;
    n = (float)L.dim;
    two_pi = c == 6.283185307179586f;  // every c that rounds to (float)(2 pi); wave-uniform: a scalar branch around the two trig forms
  }
  template <bool TWO_PI>
  __device__ __forceinline__ float body(const LaneT& L, const Slice<NV>& x, Slice<NV>& g, float& big_a) const {
    float s1 = 0.0f, s2 = 0.0f;
    Slice<NV> sn;
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float xv = x.a[v][i];
        float co;
        sincos_cx<TWO_PI>(c, xv, sn.a[v][i], co);
        const bool ok = L.ok(v, i);
        s1 += ok ? xv * xv : 0.0f;
        s2 += ok ? co : 0.0f;
      }
    s1 = group_sum<G>(s1);
    s2 = group_sum<G>(s2);
    const float r = sqrtf(s1 / n);
    const float e1 = expf(-b * r);
    const float e2 = expf(s2 / n);
    big_a = ((a * b) * e1) / (n * r);
    const float big_b = (c * e2) / n;
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        g.a[v][i] = L.ok(v, i) ? __builtin_fmaf(big_b, sn.a[v][i], big_a * x.a[v][i]) : 0.0f;
    // a (1 - e1) + (e - e2): the reference's -a e1 - e2 + a + e with the two cancelling pairs taken first
    return a * (1.0f - e1) + (2.718281828459045f - e2);
  }
  template <bool WANT_E>
  __device__ __forceinline__ float eval(const LaneT& L, const Slice<NV>& x, Slice<NV>& g) const {
    float big_a;
    const float e = two_pi ? body<true>(L, x, g, big_a) : body<false>(L, x, g, big_a);
    return WANT_E ? e : 0.0f;
  }
  __device__ __forceinline__ float eval_chk(const LaneT& L, const Slice<NV>& x, Slice<NV>& g, float& chk) const {
    float big_a;
    const float e = two_pi ? body<true>(L, x, g, big_a) : body<false>(L, x, g, big_a);
    chk = __builtin_fmaf(0.0f, big_a, e);
    return e;
  }
};

// ---------------------------------------------------------------------------------
// Rosenbrock:  E = sum_{i < n-1} (a - x_i)^2 + b r_i^2,   r_i = x_{i+1} - x_i^2
//              g_j = [j < n-1] (-2 (a - x_j) - 4 b x_j r_j)  +  [j >= 1] 2 b r_{j-1}
// Each float4 needs the first element of the vector that follows it in the row (x_{i+1} of its last column) and r of the
// last column of the vector before it: from_next / from_prev above, one exchange each per vector.  r_i is held as 0
// where term i does not exist (i >= n - 1, padded slots, chains past n_chains), which masks the energy and both
// gradient parts at once: the padded column n is never read as an x_{i+1}.
// HMC check value.  E finite => x finite (every x_i enters a square), but not => g finite: 4 b x_j r_j can overflow
// where b r_j^2 and (a - x_j)^2 do not, and inf - inf gives NaN.  eval_chk therefore tests the gradient components
// themselves: one ballot per group, chk = NaN if any is not finite.
// ---------------------------------------------------------------------------------
template <class LaneT>
struct Energy<EBM_ENERGY_ROSENBROCK, LaneT> {
  static constexpr int G = LaneT::G, NV = LaneT::NV;
  static constexpr bool HAS_GRAD_ONLY = false;
  static constexpr bool GRAD_CHECK = true;
  float a, b;
  __device__ __forceinline__ void init(const EnergyParams& P, const LaneT&, const Smem&) { a = P.s0; b = P.s1; }
  template <bool WANT_E>
  __device__ __forceinline__ float eval(const LaneT& L, const Slice<NV>& x, Slice<NV>& g) const {
    float xn[NV];  // first element of the following vector
#pragma unroll
    for (int v = 0; v < NV; ++v) xn[v] = from_next<G>(x.a[v][0], v + 1 < NV ? x.a[v + 1 < NV ? v + 1 : v][0] : 0.0f, L.lg);
    Slice<NV> r;
    float acc = 0.0f;
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float xv = x.a[v][i];
        const float nx = i < 3 ? x.a[v][i < 3 ? i + 1 : i] : xn[v];
        const bool term = L.ok(v, i) && L.col[v] + i + 1 < L.dim;
        const float rv = term ? nx - xv * xv : 0.0f;
        const float d = a - xv;
        r.a[v][i] = rv;
        g.a[v][i] = term ? -2.0f * d - (4.0f * b) * xv * rv : 0.0f;
        if (WANT_E) acc += term ? d * d + b * (rv * rv) : 0.0f;
      }
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const float rp = from_prev<G>(r.a[v][3], v > 0 ? r.a[v > 0 ? v - 1 : 0][3] : 0.0f, L.lg);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float prev = i > 0 ? r.a[v][i > 0 ? i - 1 : 0] : rp;
        const float gv = g.a[v][i] + (2.0f * b) * prev;
        g.a[v][i] = L.ok(v, i) ? gv : 0.0f;
      }
    }
    if (!WANT_E) return 0.0f;
    return group_sum<G>(acc);
  }
  __device__ __forceinline__ float eval_chk(const LaneT& L, const Slice<NV>& x, Slice<NV>& g, float& chk) const {
    const float e = eval<true>(L, x, g);
    bool bad = false;
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int i = 0; i < 4; ++i) bad = bad || !(__builtin_fabsf(g.a[v][i]) < __builtin_inff());
    chk = group_any<G>(bad) ? __builtin_nanf("") : e;
    return e;
  }
};

}  // namespace rows
}  // namespace ebm
