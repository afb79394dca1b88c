// Replica-exchange (parallel tempering) Langevin: a ladder of R tempered copies of one chain, k Euler-Maruyama steps and
// the swap events between them in ONE launch (ebm_tempering_chain_f32, include/ebm_hip.h; docs/design/tempering.md).
//
// Layout: rows.h's lane groups.  A lane group is a WALKER: it holds one state in registers from the load to the final
// store.  The R walkers of a ladder sit in consecutive groups of one workgroup (a ladder never straddles workgroups:
// LPB = (256 / G) / R ladders per block, the groups past LPB * R idle), possibly in different waves.
//
// A swap RELABELS, it does not move state: every walker carries the slot t it currently represents (and that slot's
// noise coefficient).  At a swap event the walkers post their energies to an LDS table indexed [ladder in block][slot],
// both partners of a pair read the two energies and the pair's uniform and reach the same decision, and each changes its
// own t.  Everything addressed in memory follows the SLOT: the Philox element (c * R + t) * dim + col, the injected noise
// row, the trajectory (stored by whichever walker holds slot 0) and the final store to row c * R + t.  What is physical
// -- the lane's columns, its place in the wave (the Gaussian exchange row) -- stays in the Lane that Energy::init saw.
#pragma once
#include "chain_launch.h"
#include "rows.h"
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
  const int lpb = (kBlock / G) / R;              // ladders per block
  const int walker = (int)threadIdx.x / G;       // lane group in the block
  const int lib = walker / R;                    // ladder in block
  const int64_t ladder = (int64_t)blockIdx.x * lpb + lib;
  int t = walker - lib * R;                      // the slot this walker represents now

  LaneT L;
  L.init(0, a.dim);  // columns, lane-in-group and place in the wave; the chain comes from the ladder, not the thread id
  L.active = lib < lpb && ladder < a.n_ladders;
  const int64_t row_base = L.active ? ladder * (int64_t)R : 0;
  L.chain = row_base + t;
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
  const int64_t traj_row = L.active ? ladder * (int64_t)a.n_kept * a.dim : 0;
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
      if (L.lg == 0 && lib < lpb) e_table[lib * R + t] = e_now;
      __syncthreads();
      const int parity = event & 1;
      // slot t pairs with t + 1 when t has the event's parity, with t - 1 otherwise; the ends may be unpaired
      const bool lower = ((t - parity) & 1) == 0;
      const int lo = lower ? t : t - 1;
      const bool paired = L.active && lo >= parity && lo + 1 < R;
      bool swap = false;
      if (paired) {
        const float e_lo = e_table[lib * R + lo], e_hi = e_table[lib * R + lo + 1];
        const float delta = (a.beta[lo] - a.beta[lo + 1]) * (e_lo - e_hi);
        const int64_t urow = row_base + lo;
        float uu;
        if (a.u) uu = a.u[(int64_t)event * n_rows + urow];
        else uu = u01_half_open(pick(philox_at(a.key, (uint64_t)urow >> 2, a.step0 + 2ull * (uint64_t)s + 1ull), (int)(urow & 3)));
        swap = delta == delta && uu < expf(fminf(delta, 0.0f));
      }
      if (a.swap_counts) {  // one ballot and one atomic per wave and pair, counted by the leader lane of the lower slot's walker
        const bool counts = paired && lower && L.lg == 0;
        for (int p = parity; p + 1 < R; p += 2) {
          const unsigned long long tried = __ballot(counts && lo == p);
          if (tried == 0ull) continue;
          const unsigned long long took = __ballot(counts && lo == p && swap);
          if ((threadIdx.x & 63) == 0) {
            atomicAdd(a.swap_counts + p, (uint32_t)__popcll(tried));
            if (took) atomicAdd(a.swap_counts + (R - 1) + p, (uint32_t)__popcll(took));
          }
        }
      }
      __syncthreads();  // the table is read: the next event may overwrite it
      if (swap) {
        t = lower ? t + 1 : t - 1;
        A.chain = row_base + t;
        noise_coef = a.noise_coef[t];
      }
      ++event;
    }

    if (a.traj && --until_keep == 0) {
      until_keep = a.thin;
      if (t == 0) store_slice(A, a.traj, traj_row + keep_off, x);
      keep_off += a.dim;
    }
  }
  store_slice(A, a.x, A.chain * (int64_t)a.dim, x);
}

template <int KIND>
void launch_kind(const Geometry& geo, dim3 grid, size_t smem, hipStream_t st, const TemperArgs& a) {
  EBM_GEO_LAUNCH(tempering_ladder_chain, KIND, geo, grid, dim3(kBlock), smem, st, a);
}

}  // namespace

}  // namespace tempering
}  // namespace ebm
