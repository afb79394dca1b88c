// Underdamped (kinetic) Langevin dynamics in the BAOAB splitting: a walker per chain that keeps position, velocity and the
// carried gradient in registers from the load to the one store (ebm_kinetic_chain_f32, include/ebm_hip.h;
// docs/design/kinetic.md).
//
// Layout: rows.h -- a lane group is a chain; x, v and g are one slice each, 12 registers per lane.  A chain never talks to
// another: no exchange and no barrier in the loop beyond what Energy::eval needs; hh, c1, c2 and the thinning test are
// wave-uniform.  One gradient evaluation per step, the start's in front of the loop.
#pragma once
#include "chain_launch.h"
#include "landscape_energies.h"
#include "rows.h"

namespace ebm {
namespace kinetic {
using namespace rows;

struct KineticArgs {
  float* x;            // [n_chains, dim], in/out
  float* v;            // [n_chains, dim]: in/out, output only with draw_v0
  int64_t n_chains;
  int32_t dim, k_steps, thin, n_kept, draw_v0;
  float hh, c1, c2, sqrt_temp;
  float* traj;         // [n_chains, n_kept, dim] or null
  const float* noise;  // [k_steps, n_chains, dim] or null
  RngKey key;
  uint64_t step0;
  EnergyParams energy;
  int param_floats;
};

namespace {

extern __shared__ __attribute__((aligned(16))) float kinetic_smem[];

template <int KIND, int G, int NV, bool FULL>
__global__ __launch_bounds__(kBlock) void kinetic_chain(KineticArgs a) {
  static_assert(NV == 1, "one vector per lane");
  using LaneT = Lane<G, 1, FULL>;
  LaneT L;
  L.init(a.n_chains, a.dim);
  const Smem S = carve_smem<1>(kinetic_smem, a.param_floats);
  stage_params(a.energy, a.dim, S.param);
  Energy<KIND, LaneT> en;
  en.init(a.energy, L, S);

  const int64_t row = L.active ? L.chain * (int64_t)a.dim : 0;
  const int64_t traj_row = L.active ? L.chain * (int64_t)a.n_kept * a.dim : 0;
  const float hh = a.hh, c1 = a.c1, c2 = a.c2;
  Slice<1> x, v, g;
  load_slice(L, a.x, row, x);
  if (a.draw_v0) {  // wave-uniform
    normal_slice(L, a.key, a.step0, v);
#pragma unroll
    for (int i = 0; i < 4; ++i) v.a[0][i] = L.ok(0, i) ? a.sqrt_temp * v.a[0][i] : 0.0f;
  } else {
    load_slice(L, a.v, row, v);
  }
  en.template eval<false>(L, x, g);  // the raw gradient, no clamp: a NaN stays in its chain

  int kept = 0, until_keep = a.thin;
  for (int s = 0; s < a.k_steps; ++s) {
    Slice<1> xi;
    if (a.noise) load_slice(L, a.noise, ((int64_t)s * a.n_chains) * a.dim + row, xi);
    else normal_slice(L, a.key, a.step0 + 1ull + (uint64_t)s, xi);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      // B, A, O, A: every operation rounded on its own
      float vi = v.a[0][i] - hh * g.a[0][i];
      float xv = x.a[0][i] + hh * vi;
      vi = c1 * vi + c2 * xi.a[0][i];
      xv = xv + hh * vi;
      x.a[0][i] = L.ok(0, i) ? xv : 0.0f;
      v.a[0][i] = L.ok(0, i) ? vi : 0.0f;
    }
    en.template eval<false>(L, x, g);
#pragma unroll
    for (int i = 0; i < 4; ++i) {  // B
      const float vi = v.a[0][i] - hh * g.a[0][i];
      v.a[0][i] = L.ok(0, i) ? vi : 0.0f;
    }
    if (--until_keep == 0) {  // wave-uniform: (s + 1) % thin == 0
      until_keep = a.thin;
      if (a.traj && kept < a.n_kept) store_slice(L, a.traj, traj_row + (int64_t)kept * a.dim, x);
      ++kept;
    }
  }
  store_slice(L, a.x, row, x);
  store_slice(L, a.v, row, v);
}

}  // namespace

// The launcher of one energy kind: defined and instantiated in kinetic_unit.hip (one object per kind).
template <int KIND>
void launch_kind(const Geometry& geo, dim3 grid, size_t smem, hipStream_t st, const KineticArgs& a);

}  // namespace kinetic
}  // namespace ebm
