// Annealed importance sampling: one chain walks ONE state from the base N(0, sigma0^2 I) to the target through T tempered
// laws, a Metropolis-corrected HMC transition at each, and accumulates the importance weight -- the whole walk in ONE launch
// (ebm_ais_chain_f32, include/ebm_hip.h; docs/design/ais.md).
//
// Layout: rows.h -- a lane group is a chain that keeps its state in registers from the draw (or the load of the injected start)
// to the one store at the end.  The replica-exchange kernels (tempering_hmc_kernel.h) run R temperatures side by side and swap
// labels through LDS; here the temperatures follow each other in time, so a chain never talks to another: no exchange, no
// barrier in the loop, beta[t] and eps[t] are wave-uniform loads.
//
// Transition: ebm_hmc_chain_f32's (hmc_kernel.h: leapfrog_steps<false>, IdentityKinetic, metropolis_accept; the accept uniform is
// spelled here as hmc_chain_body spells it), on the PATH energy
//   U_b(x) = (1 - b) E_0(x) + b E(x),   E_0(x) = 0.5 inv_var0 sum x^2
// which PathEnergy hands it as an Energy of its own around the kind's: one evaluation of the kind's energy gives U and dU/dx,
// and the adapter keeps E, E_0 and the raw dE/dx of its LAST evaluation -- the proposal's.  Those three are what a chain
// carries: the weight update  logw += (b_t - b_{t-1}) (E_0 - E)  evaluates nothing, H0 is the mix of the carried energies at
// the new b, and the force the trajectory starts from is rebuilt from the carried raw gradient (b changed, so the clamped
// force of the last trajectory is of no use).  A transition costs n_leapfrog evaluations, like ebm_hmc_chain_f32's.
// The mix is (1 - b) * a + b * c in separately rounded operations and nothing is ever divided by b: at b = 1 it is
// 0 * a + 1 * c = c exactly, and the transition is that of hmc_chain_body on the same lane geometry bit for bit.
#pragma once
#include "chain_launch.h"
#include "hmc_kernel.h"
#include "landscape_energies.h"

namespace ebm {
namespace ais {
using namespace rows;

struct AisArgs {
  float* x;                 // [n_chains, dim], written once
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
  EnergyParams energy;
  int param_floats;
};

// GRAD_CHECK of the kind's energy (rows.h has_grad_check) shows through the adapter
template <class Inner, bool = has_grad_check<Inner>::value>
struct GradCheckOf {};
template <class Inner>
struct GradCheckOf<Inner, true> {
  static constexpr bool GRAD_CHECK = true;
};

// U_b as an Energy<>: what leapfrog_steps evaluates.  `mutable`: leapfrog_steps takes its energy const, and the parts of the
// last evaluation are this adapter's second result.
template <class Inner, class LaneT>
struct PathEnergy : GradCheckOf<Inner> {
  static constexpr int G = LaneT::G, NV = LaneT::NV;
  static constexpr bool HAS_GRAD_ONLY = Inner::HAS_GRAD_ONLY;
  const Inner& in;
  float half_inv_var0, inv_var0;
  float b0, b1, c0;  // 1 - b, b, (1 - b) inv_var0
  mutable float e_tgt, e_base;  // E and E_0 of the last evaluation with the energy
  mutable Slice<NV> g_tgt;      // its raw dE/dx

  __device__ __forceinline__ PathEnergy(const Inner& inner, float inv_var0_)
      : in(inner), half_inv_var0(0.5f * inv_var0_), inv_var0(inv_var0_), b0(0.0f), b1(1.0f), c0(0.0f), e_tgt(0.0f), e_base(0.0f) {}
  __device__ __forceinline__ void set_beta(float b) {
    b1 = b;
    b0 = 1.0f - b;
    c0 = b0 * inv_var0;
  }
  __device__ __forceinline__ float mix_energy(float e0, float e) const { return b0 * e0 + b1 * e; }
  // dU/dx from the raw dE/dx; slots that hold no column have x = 0 and g = 0 and stay 0
  __device__ __forceinline__ void mix_grad(const Slice<NV>& x, const Slice<NV>& g_raw, Slice<NV>& g) const {
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int i = 0; i < 4; ++i) g.a[v][i] = c0 * x.a[v][i] + b1 * g_raw.a[v][i];
  }
  __device__ __forceinline__ float base_energy(const LaneT& L, const Slice<NV>& x) const {
    float acc = 0.0f;
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float sq = x.a[v][i] * x.a[v][i];
        acc += L.ok(v, i) ? sq : 0.0f;
      }
    return half_inv_var0 * group_sum<G>(acc);
  }
  __device__ __forceinline__ float keep(const LaneT& L, const Slice<NV>& x, const Slice<NV>& g_raw, float e) const {
    e_tgt = e;
    e_base = base_energy(L, x);
    g_tgt = g_raw;
    return mix_energy(e_base, e);
  }

  template <bool WANT_E>
  __device__ __forceinline__ float eval(const LaneT& L, const Slice<NV>& x, Slice<NV>& g) const {
    Slice<NV> g_raw;
    const float e = in.template eval<WANT_E>(L, x, g_raw);
    mix_grad(x, g_raw, g);
    if constexpr (!WANT_E) return 0.0f;
    return keep(L, x, g_raw, e);
  }
  // (HAS_GRAD_ONLY kinds) the check value is the kind's own: finite => x finite and dE/dx free of NaN, and then so is dU/dx
  __device__ __forceinline__ bool grad_only_ready() const { return in.grad_only_ready(); }
  __device__ __forceinline__ float grad_only(const LaneT& L, const Slice<NV>& x, Slice<NV>& g) const {
    Slice<NV> g_raw;
    const float chk = in.grad_only(L, x, g_raw);
    mix_grad(x, g_raw, g);
    return chk;
  }
  // (GRAD_CHECK kinds) the kind's check value vouches for dE/dx, U for the rest
  __device__ __forceinline__ float eval_chk(const LaneT& L, const Slice<NV>& x, Slice<NV>& g, float& chk) const {
    Slice<NV> g_raw;
    float chk_in;
    const float e = in.eval_chk(L, x, g_raw, chk_in);
    mix_grad(x, g_raw, g);
    const float u = keep(L, x, g_raw, e);
    chk = (__builtin_fabsf(chk_in) < __builtin_inff()) ? u : chk_in;
    return u;
  }
};

namespace {

extern __shared__ __attribute__((aligned(16))) float ais_smem[];

// One vector per lane (dim <= 256), the geometry of pick_geometry: ais_unit.hip builds no other.
template <int KIND, int G, int NV, bool FULL>
__global__ __launch_bounds__(kBlock) void ais_chain(AisArgs a) {
  static_assert(NV == 1, "one vector per lane");
  using LaneT = Lane<G, NV, FULL>;
  LaneT L;
  L.init(a.n_chains, a.dim);
  const Smem S = carve_smem<NV>(ais_smem, a.param_floats);
  stage_params(a.energy, a.dim, S.param);
  Energy<KIND, LaneT> en;
  en.init(a.energy, L, S);
  PathEnergy<Energy<KIND, LaneT>, LaneT> path(en, a.inv_var0);

  const int64_t row = L.active ? L.chain * (int64_t)a.dim : 0;
  const bool leader = L.active && L.lg == 0;

  // ---- start: the injected state, or sigma0 z
  Slice<NV> xc;
  if (a.x0) {
    load_slice(L, a.x0, row, xc);
  } else {
    normal_slice(L, a.key, a.step0, xc);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float xv = a.sigma0 * xc.a[0][i];
      xc.a[0][i] = L.mem_ok(0, i) ? xv : 0.0f;
    }
  }

  const hmc::IdentityKinetic<LaneT> kinetic{L};

  // what the chain carries besides its state: E, E_0 and the raw dE/dx there.  Those of the start come out of the
  // pseudo-transition t = 0 (hmc_kernel.h: zero momentum, zero step size, one leapfrog step, always taken), so the energy is
  // inlined at one call site.
  float e_cur = 0.0f, e0_cur = 0.0f;
  Slice<NV> g_cur;
#pragma unroll
  for (int i = 0; i < 4; ++i) g_cur.a[0][i] = 0.0f;
  float lw = 0.0f, lw_c = 0.0f;  // the weight: a Kahan pair
  float beta_prev = a.beta[0];

  for (int t = 0; t <= a.n_temps; ++t) {
    const bool init = t == 0;
    const float beta_t = init ? 1.0f : a.beta[t];  // wave-uniform
    const float eps_t = init ? 0.0f : a.eps[t - 1];
    const float half_eps = 0.5f * eps_t;

    // ---- the weight, from the carried energies
    if (!init) {
      const float term = (beta_t - beta_prev) * (e0_cur - e_cur);
      const float y = term - lw_c;
      const float s = lw + y;
      lw_c = (__builtin_fabsf(s) < __builtin_inff()) ? (s - lw) - y : 0.0f;  // an infinite sum stays what a plain sum gives
      lw = s;
      beta_prev = beta_t;
    }
    path.set_beta(beta_t);

    // ---- the force of U_{beta_t} at the held state, from the carried raw gradient (NaN-propagating, as the reference's clamp_)
    Slice<NV> f;
    path.mix_grad(xc, g_cur, f);
#pragma unroll
    for (int i = 0; i < 4; ++i) f.a[0][i] = init ? 0.0f : clamp_nanprop(-f.a[0][i], -1e6f, 1e6f);  // (t = 0: as hmc_chain_body starts)

    // ---- momentum draw
    Slice<NV> p;
    if (init) {
#pragma unroll
      for (int i = 0; i < 4; ++i) p.a[0][i] = 0.0f;
    } else {
      if (a.p_noise) load_slice(L, a.p_noise, ((int64_t)(t - 1) * a.n_chains) * a.dim + row, p);
      else normal_slice(L, a.key, a.step0 + 2ull * (uint64_t)t - 1ull, p);
#pragma unroll
      for (int i = 0; i < 4; ++i) p.a[0][i] = L.ok(0, i) ? p.a[0][i] : 0.0f;
    }

    // ---- the accept uniform, drawn in front of the trajectory as in hmc_chain_body
    float uu;
    if (init) uu = -1.0f;
    else if (a.u_accept) uu = L.active ? a.u_accept[(int64_t)(t - 1) * a.n_chains + L.chain] : 2.0f;
    else uu = u01_half_open(pick(philox_at(a.key, (uint64_t)L.chain >> 2, a.step0 + 2ull * (uint64_t)t), (int)(L.chain & 3)));

    // ---- H0 from the carried energies
    const float u0 = path.mix_energy(e0_cur, e_cur);
    const float h0 = clamp_nanprop(u0, -1e10f, 1e10f) + kinetic(p);

    // ---- proposal
    Slice<NV> x = xc;
    const int n_lf = init ? 1 : a.n_leapfrog;
    const float u1 = hmc::leapfrog_steps<false>(path, L, x, p, f, x, eps_t, half_eps, n_lf, u0, init);
    const float h1 = clamp_nanprop(u1, -1e10f, 1e10f) + kinetic(p);

    // ---- Metropolis accept
    const bool accept = hmc::metropolis_accept(h0 - h1, uu, init, L.active);
    if (accept) {  // the proposal's parts become the carried ones
      xc = x;
      e_cur = path.e_tgt;
      e0_cur = path.e_base;
      g_cur = path.g_tgt;
    }
    if (init) continue;

    if (a.accept_mask && leader) a.accept_mask[(int64_t)(t - 1) * a.n_chains + L.chain] = accept ? 1 : 0;
    if (a.accept_counts) {  // one ballot and one atomic per wave and temperature
      const unsigned long long b = __ballot(accept && leader);
      if ((threadIdx.x & 63) == 0 && b) atomicAdd(a.accept_counts + (t - 1), (uint32_t)__popcll(b));
    }
  }
  store_slice(L, a.x, row, xc);
  if (leader) a.logw[L.chain] = lw;
}

}  // namespace

// The launcher of one energy kind: defined and instantiated in ais_unit.hip (one object per kind).
template <int KIND>
void launch_kind(const Geometry& geo, dim3 grid, size_t smem, hipStream_t st, const AisArgs& a);

}  // namespace ais
}  // namespace ebm
