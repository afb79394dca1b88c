// Replica-exchange HMC: a ladder of R tempered copies of one chain, n_mh Metropolis-corrected HMC transitions of every copy
// and the swap events between them in ONE launch (ebm_tempering_hmc_chain_f32, include/ebm_hip.h;
// docs/design/tempering_hmc.md).
//
// Layout, label swapping and the swap event: ladder.h -- a lane group is a WALKER that keeps one state in registers from the load
// to the final store, a swap changes the slot a walker represents, and everything addressed in memory (Philox elements, injected
// draws, the accept mask, the trajectory, the final store) follows the slot through the addressing view A while the energies
// read the physical lane L.
//
// Transition: ebm_hmc_chain_f32's -- the trajectory is hmc::leapfrog_steps<false> of hmc_kernel.h (the carried energy and
// force, the pseudo-transition t = -1, the merged kicks, the literal fallback), the kinetic energy and the Metropolis decision
// are its helpers (IdentityKinetic, metropolis_accept), and the accept uniform is spelled here as hmc_chain_body spells it;
// this kernel puts the slot's temperature in.  Slot r samples
// exp(-beta_r E) with the mass beta_r I: in the velocity variable w = p / beta_r that is the leapfrog on E itself with
// w ~ N(0, T_r), and the Hamiltonian difference is beta_r (H0 - H1).  Nothing a walker carries -- x, E(x), the clamped force --
// depends on its temperature, so a swap event posts the carried energies and evaluates nothing; the walker changes its slot,
// its row, eps, sqrt_temp and beta.
#pragma once
#include "chain_launch.h"
#include "hmc_kernel.h"
#include "ladder.h"
#include "landscape_energies.h"

namespace ebm {
namespace tempering_hmc {
using namespace rows;

struct TemperHmcArgs {
  float* x;                 // [n_ladders * R, dim]
  int64_t n_ladders;
  int32_t R, dim, n_mh, n_leapfrog;
  const float* eps;         // device [R]
  const float* sqrt_temp;   // device [R]
  const float* beta;        // device [R]
  int32_t swap_every, thin, n_kept;
  float* traj;              // [n_ladders, n_kept, dim] or null
  uint8_t* accept_mask;     // [n_mh, n_ladders * R] or null
  uint32_t* accept_counts;  // [R]: accepted proposals of each slot; or null
  uint32_t* swap_counts;    // [2 * (R - 1)]: attempts of pair (p, p + 1) at p, accepts at R - 1 + p; or null
  const float* p_noise;     // [n_mh, n_ladders * R, dim] or null
  const float* u_accept;    // [n_mh, n_ladders * R] or null
  const float* u_swap;      // [n_events, n_ladders * R] or null
  RngKey key;
  uint64_t step0;
  EnergyParams energy;
  int param_floats;
  int table_offset_floats;  // start of the energy table in dynamic LDS; the per-slot accept counters sit behind it
};

namespace {

extern __shared__ __attribute__((aligned(16))) float temper_hmc_smem[];

// One vector per lane (dim <= 256), the geometry of pick_geometry: tempering_hmc_unit.hip builds no other.
template <int KIND, int G, int NV, bool FULL>
__global__ __launch_bounds__(kBlock) void tempering_hmc_ladder_chain(TemperHmcArgs a) {
  static_assert(NV == 1, "one vector per lane");
  using LaneT = Lane<G, NV, FULL>;
  const int R = a.R;
  LaneT L;
  const ladder::Place w = ladder::place_walker(L, R, a.dim, a.n_ladders);
  int r = w.slot;  // the slot this walker represents now
  // the validity mask for the ladder's own `active`; why here and not in place_walker: docs/design/tempering.md, Limits
  L.valid = 0;
#pragma unroll
  for (int v = 0; v < NV; ++v)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (L.active && L.col[v] + i < a.dim) L.valid |= 1u << (v * 4 + i);

  // dynamic LDS behind the energy parameters: [kBlock / G] energies indexed lib * R + slot, then [R] accept counters
  // (indexed straight off the LDS array, like the parking slots of hmc_kernel.h)
  const int e_table = a.table_offset_floats;
  uint32_t* acc_table = reinterpret_cast<uint32_t*>(&temper_hmc_smem[a.table_offset_floats + kBlock / G]);
  if (a.accept_counts && (int)threadIdx.x < R) acc_table[threadIdx.x] = 0u;
  __syncthreads();

  const Smem S = carve_smem<NV>(temper_hmc_smem, a.param_floats);
  stage_params(a.energy, a.dim, S.param);
  Energy<KIND, LaneT> en;
  en.init(a.energy, L, S);

  LaneT A = L;  // the addressing view: A.chain is the SLOT's row and changes with r
  Slice<NV> xc;
  load_slice(A, a.x, A.chain * (int64_t)a.dim, xc);
  float eps = a.eps[r], sqrt_temp = a.sqrt_temp[r], beta = a.beta[r];
  const int64_t n_rows = a.n_ladders * (int64_t)R;
  const int64_t traj_row = L.active ? w.ladder * (int64_t)a.n_kept * a.dim : 0;
  const bool leader = L.active && L.lg == 0;
  int until_keep = a.thin, until_swap = a.swap_every;
  int64_t keep_off = 0;
  int event = 0;

  const hmc::IdentityKinetic<LaneT> kinetic{L};

  // energy and clamped force of the state the walker holds, carried from transition to transition and through every swap;
  // the pair of the initial state comes out of the pseudo-transition t = -1 (hmc_kernel.h)
  Slice<NV> f;
#pragma unroll
  for (int i = 0; i < 4; ++i) f.a[0][i] = 0.0f;
  float e_cur = 0.0f;

  for (int t = -1; t < a.n_mh; ++t) {
    const bool init = t < 0;
    const float eps_t = init ? 0.0f : eps;
    const float half_eps = 0.5f * eps_t;

    // ---- velocity draw: w = z sqrt(T_r)
    Slice<NV> p;
    if (init) {
#pragma unroll
      for (int i = 0; i < 4; ++i) p.a[0][i] = 0.0f;
    } else {
      if (a.p_noise) load_slice(A, a.p_noise, ((int64_t)t * n_rows + A.chain) * a.dim, p);
      else normal_slice(A, a.key, a.step0 + 3ull * (uint64_t)t, p);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float pv = p.a[0][i] * sqrt_temp;
        p.a[0][i] = L.ok(0, i) ? pv : 0.0f;
      }
    }

    // ---- the accept uniform of the slot's row, drawn in front of the trajectory as in hmc_chain_body
    float uu;
    if (init) uu = -1.0f;
    else if (a.u_accept) uu = L.active ? a.u_accept[(int64_t)t * n_rows + A.chain] : 2.0f;
    else uu = u01_half_open(pick(philox_at(a.key, (uint64_t)A.chain >> 2, a.step0 + 3ull * (uint64_t)t + 1ull),
                                 (int)(A.chain & 3)));

    // ---- H0 from the carried energy
    const float e0 = e_cur;
    const float h0 = clamp_nanprop(e0, -1e10f, 1e10f) + kinetic(p);

    // ---- proposal
    Slice<NV> f_keep = f;
    Slice<NV> x = xc;
    const int n_lf = init ? 1 : a.n_leapfrog;
    const float e1 = hmc::leapfrog_steps<false>(en, L, x, p, f, x, eps_t, half_eps, n_lf, e0, init);
    const float h1 = clamp_nanprop(e1, -1e10f, 1e10f) + kinetic(p);

    // ---- Metropolis accept at the slot's temperature: the Hamiltonian of (x, p = beta w) with M = beta I is beta (E + K(w))
    const bool accept = hmc::metropolis_accept(beta * (h0 - h1), uu, init, L.active);
    if (accept) {
      e_cur = e1;
      xc = x;
    } else {
      f = f_keep;
    }
    if (init) continue;

    if (a.accept_mask && leader) a.accept_mask[(int64_t)t * n_rows + A.chain] = accept ? 1 : 0;
    if (a.accept_counts && leader && accept) atomicAdd(&acc_table[r], 1u);  // LDS; one global atomic per slot and block at the end

    if (--until_swap == 0) {  // uniform: every thread of the block reaches both barriers
      until_swap = a.swap_every;
      const ladder::SwapDraws draws{a.u_swap, a.key, a.step0 + 3ull * (uint64_t)t + 2ull};
      // the carried energy is posted: nothing is evaluated.  The labels change; x, e_cur and f stay
      if (ladder::swap_event(L, w, R, n_rows, event, r, A.chain, &temper_hmc_smem[e_table], e_cur, a.beta, draws, a.swap_counts)) {
        eps = a.eps[r];
        sqrt_temp = a.sqrt_temp[r];
        beta = a.beta[r];
      }
    }

    if (a.traj && --until_keep == 0) {
      until_keep = a.thin;
      if (r == 0) store_slice(A, a.traj, traj_row + keep_off, xc);
      keep_off += a.dim;
    }
  }
  store_slice(A, a.x, A.chain * (int64_t)a.dim, xc);
  if (a.accept_counts) {
    __syncthreads();
    if ((int)threadIdx.x < R && acc_table[threadIdx.x]) atomicAdd(a.accept_counts + threadIdx.x, acc_table[threadIdx.x]);
  }
}

}  // namespace

// The launcher of one energy kind: defined and instantiated in tempering_hmc_unit.hip (one object per kind).
template <int KIND>
void launch_kind(const Geometry& geo, dim3 grid, size_t smem, hipStream_t st, const TemperHmcArgs& a);

}  // namespace tempering_hmc
}  // namespace ebm
