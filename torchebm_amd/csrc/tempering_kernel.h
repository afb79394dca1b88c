// Replica-exchange (parallel tempering) Langevin: a ladder of R tempered copies of one chain, k Euler-Maruyama steps and
// the swap events between them in ONE launch (ebm_tempering_chain_f32, include/ebm_hip.h; docs/design/tempering.md).
//
// Layout, label swapping and the swap event: ladder.h.  What is this kernel's own: the Euler-Maruyama step with the slot's
// noise coefficient, and the energy evaluation in front of a swap (a Langevin walker carries no energy).
#pragma once
#include "chain_launch.h"
#include "ladder.h"
#include "landscape_energies.h"

namespace ebm {
namespace tempering {
using namespace rows;

struct TemperArgs {
  float* x;                 // [n_ladders * R, dim]
  int64_t n_ladders;
  int32_t R, dim, k_steps;
  float eta, sqrt_eta;
  const float* noise_coef;  // device [R]
  const float* beta;        // device [R]
  int32_t swap_every, thin, n_kept;
  float* traj;              // [n_ladders, n_kept, dim] or null
  uint32_t* swap_counts;    // [2 * (R - 1)]: attempts of pair (p, p + 1) at p, accepts at R - 1 + p; or null
  const float* noise;       // [k, n_ladders * R, dim] or null
  const float* u;           // [n_events, n_ladders * R] or null
  RngKey key;
  uint64_t step0;
  EnergyParams energy;
  int param_floats;
  int table_offset_floats;  // start of the energy table in dynamic LDS
};

namespace {

extern __shared__ __attribute__((aligned(16))) float temper_smem[];

template <int KIND, int G, int NV, bool FULL>
__global__ __launch_bounds__(kBlock) void tempering_ladder_chain(TemperArgs a) {
  using LaneT = Lane<G, NV, FULL>;
  const int R = a.R;
  LaneT L;
  const ladder::Place w = ladder::place_walker(L, R, a.dim, a.n_ladders);
  int t = w.slot;  // the slot this walker represents now
  // the validity mask for the ladder's own `active`; why here and not in place_walker: docs/design/tempering.md, Limits
  L.valid = 0;
#pragma unroll
  for (int v = 0; v < NV; ++v)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (L.active && L.col[v] + i < a.dim) L.valid |= 1u << (v * 4 + i);

  const Smem S = carve_smem<NV>(temper_smem, a.param_floats);
  stage_params(a.energy, a.dim, S.param);
  Energy<KIND, LaneT> en;
  en.init(a.energy, L, S);
  float* e_table = temper_smem + a.table_offset_floats;  // [kBlock / G] energies, indexed lib * R + slot

  LaneT A = L;  // the addressing view: A.chain is the SLOT's row and changes with t
  Slice<NV> x;
  load_slice(A, a.x, A.chain * (int64_t)a.dim, x);
  float noise_coef = a.noise_coef[t];
  const int64_t n_rows = a.n_ladders * (int64_t)R;
  const int64_t traj_row = L.active ? w.ladder * (int64_t)a.n_kept * a.dim : 0;
  const float eta = a.eta, sqrt_eta = a.sqrt_eta;
  int until_keep = a.thin, until_swap = a.swap_every;
  int64_t keep_off = 0;
  int event = 0;

  for (int s = 0; s < a.k_steps; ++s) {
    Slice<NV> g, eps;
    en.template eval<false>(L, x, g);
    if (a.noise) load_slice(A, a.noise, ((int64_t)s * n_rows + A.chain) * a.dim, eps);
    else normal_slice(A, a.key, a.step0 + 2ull * (uint64_t)s, eps);
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        // the reference's op order, as rows_langevin.hip: rounded mul, rounded add
        const float x1 = x.a[v][i] - eta * g.a[v][i];
        const float dw = eps.a[v][i] * sqrt_eta;
        const float nv = x1 + noise_coef * dw;
        x.a[v][i] = L.ok(v, i) ? nv : 0.0f;
      }

    if (--until_swap == 0) {  // uniform: every thread of the block reaches both barriers
      until_swap = a.swap_every;
      Slice<NV> g_unused;
      const float e_now = en.template eval<true>(L, x, g_unused);
      const ladder::SwapDraws draws{a.u, a.key, a.step0 + 2ull * (uint64_t)s + 1ull};
      if (ladder::swap_event(L, w, R, n_rows, event, t, A.chain, e_table, e_now, a.beta, draws, a.swap_counts)) noise_coef = a.noise_coef[t];
    }

    if (a.traj && --until_keep == 0) {
      until_keep = a.thin;
      if (t == 0) store_slice(A, a.traj, traj_row + keep_off, x);
      keep_off += a.dim;
    }
  }
  store_slice(A, a.x, A.chain * (int64_t)a.dim, x);
}

}  // namespace

// The launcher of one energy kind: defined and instantiated in tempering_unit.hip (one object per kind).
template <int KIND>
void launch_kind(const Geometry& geo, dim3 grid, size_t smem, hipStream_t st, const TemperArgs& a);

}  // namespace tempering
}  // namespace ebm
