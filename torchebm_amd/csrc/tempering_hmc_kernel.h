// Replica-exchange HMC: a ladder of R tempered copies of one chain, n_mh Metropolis-corrected HMC transitions of every copy
// and the swap events between them in ONE launch (ebm_tempering_hmc_chain_f32, include/ebm_hip.h;
// docs/design/tempering_hmc.md).
//
// Layout and label swapping: tempering_kernel.h -- a lane group is a WALKER that keeps one state in registers from the load
// to the final store, the R walkers of a ladder sit in consecutive groups of one workgroup, a swap changes the slot r a walker
// represents, and everything addressed in memory (Philox elements, injected draws, the accept mask, the trajectory, the final
// store) follows the slot through the addressing view A while the energies read the physical lane L.
//
// Transition: the trajectory is hmc::leapfrog_steps<false> of hmc_kernel.h, so the carried energy and force, the
// pseudo-transition t = -1, the merged kicks and the literal fallback are those of ebm_hmc_chain_f32; the arithmetic around it
// (draw, H0, H1, accept) is restated here with the slot's temperature in it.  Slot r samples exp(-beta_r E) with the mass
// beta_r I: in the velocity variable w = p / beta_r that is the leapfrog on E itself with w ~ N(0, T_r), and the Hamiltonian
// difference is beta_r (H0 - H1).  Nothing a walker carries -- x, E(x), the clamped force -- depends on its temperature, so a
// swap event posts the carried energies and evaluates nothing; the walker changes r, its row, eps, sqrt_temp and beta.
#pragma once
#include "chain_launch.h"
#include "hmc_kernel.h"
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

// One vector per lane (dim <= 256): the geometry of pick_geometry.
template <int KIND, int G, bool FULL>
__global__ __launch_bounds__(kBlock) void tempering_hmc_ladder_chain(TemperHmcArgs a) {
  constexpr int NV = 1;
  using LaneT = Lane<G, NV, FULL>;
  const int R = a.R;
  const int lpb = (kBlock / G) / R;              // ladders per block
  const int walker = (int)threadIdx.x / G;       // lane group in the block
  const int lib = walker / R;                    // ladder in block
  const int64_t ladder = (int64_t)blockIdx.x * lpb + lib;
  int r = walker - lib * R;                      // the slot this walker represents now

  LaneT L;
  L.init(0, a.dim);  // columns, lane-in-group and place in the wave; the chain comes from the ladder, not the thread id
  L.active = lib < lpb && ladder < a.n_ladders;
  const int64_t row_base = L.active ? ladder * (int64_t)R : 0;
  L.chain = row_base + r;
  L.valid = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (L.active && L.col[0] + i < a.dim) L.valid |= 1u << i;

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
  const int64_t traj_row = L.active ? ladder * (int64_t)a.n_kept * a.dim : 0;
  const bool leader = L.active && L.lg == 0;
  int until_keep = a.thin, until_swap = a.swap_every;
  int64_t keep_off = 0;
  int event = 0;

  // K(w) = 0.5 sum w^2, clamped to [0, 1e10]: the identity-mass form of hmc_chain_body
  auto kinetic = [&](const Slice<NV>& q) -> float {
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float sq = q.a[0][i] * q.a[0][i];
      acc += L.ok(0, i) ? sq : 0.0f;
    }
    return clamp_nanprop(0.5f * group_sum<G>(acc), 0.0f, 1e10f);
  };

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
    const float dlt = clamp_nanprop(beta * (h0 - h1), -50.0f, 50.0f);
    float acc_p = expf(dlt);
    acc_p = (acc_p > 1.0f) ? 1.0f : acc_p;  // NaN stays NaN and rejects
    const bool accept = init || (L.active && (uu < acc_p));
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
      if (L.lg == 0 && lib < lpb) temper_hmc_smem[e_table + lib * R + r] = e_cur;  // the carried energy: nothing is evaluated
      __syncthreads();
      const int parity = event & 1;
      // slot r pairs with r + 1 when r has the event's parity, with r - 1 otherwise; the ends may be unpaired
      const bool lower = ((r - parity) & 1) == 0;
      const int lo = lower ? r : r - 1;
      const bool paired = L.active && lo >= parity && lo + 1 < R;
      bool swap = false;
      if (paired) {
        const float e_lo = temper_hmc_smem[e_table + lib * R + lo], e_hi = temper_hmc_smem[e_table + lib * R + lo + 1];
        const float delta = (a.beta[lo] - a.beta[lo + 1]) * (e_lo - e_hi);
        const int64_t urow = row_base + lo;
        float us;
        if (a.u_swap) us = a.u_swap[(int64_t)event * n_rows + urow];
        else us = u01_half_open(pick(philox_at(a.key, (uint64_t)urow >> 2, a.step0 + 3ull * (uint64_t)t + 2ull), (int)(urow & 3)));
        swap = delta == delta && us < expf(fminf(delta, 0.0f));
      }
      if (a.swap_counts) {  // one ballot and one atomic per wave and pair, counted by the leader lane of the lower slot's walker
        const bool counts = paired && lower && L.lg == 0;
        for (int q = parity; q + 1 < R; q += 2) {
          const unsigned long long tried = __ballot(counts && lo == q);
          if (tried == 0ull) continue;
          const unsigned long long took = __ballot(counts && lo == q && swap);
          if ((threadIdx.x & 63) == 0) {
            atomicAdd(a.swap_counts + q, (uint32_t)__popcll(tried));
            if (took) atomicAdd(a.swap_counts + (R - 1) + q, (uint32_t)__popcll(took));
          }
        }
      }
      __syncthreads();  // the table is read: the next event may overwrite it
      if (swap) {  // the labels change; x, e_cur and f stay
        r = lower ? r + 1 : r - 1;
        A.chain = row_base + r;
        eps = a.eps[r];
        sqrt_temp = a.sqrt_temp[r];
        beta = a.beta[r];
      }
      ++event;
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

template <int KIND>
void launch_kind(const Geometry& geo, dim3 grid, size_t smem, hipStream_t st, const TemperHmcArgs& a) {
  const dim3 block(kBlock);
#define EBM_TEMPER_HMC_G(GV)                                                                                          \
  case GV:                                                                                                            \
    if (geo.full) hipLaunchKernelGGL((tempering_hmc_ladder_chain<KIND, GV, true>), grid, block, smem, st, a);         \
    else hipLaunchKernelGGL((tempering_hmc_ladder_chain<KIND, GV, false>), grid, block, smem, st, a);                 \
    break;
  switch (geo.G) {
    EBM_TEMPER_HMC_G(1) EBM_TEMPER_HMC_G(2) EBM_TEMPER_HMC_G(4) EBM_TEMPER_HMC_G(8) EBM_TEMPER_HMC_G(16) EBM_TEMPER_HMC_G(32)
    EBM_TEMPER_HMC_G(64)
  }
#undef EBM_TEMPER_HMC_G
}

}  // namespace

}  // namespace tempering_hmc
}  // namespace ebm
