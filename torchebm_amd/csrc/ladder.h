// The ladder of the replica-exchange kernels (tempering_kernel.h, tempering_hmc_kernel.h): who a lane group is, where its
// ladder's rows start, and the swap event -- written once, so both kernels take the same swap decisions by construction.
//
// Layout: rows.h's lane groups.  A lane group is a WALKER: it holds one state in registers from the load to the final
// store.  The R walkers of a ladder sit in consecutive groups of one workgroup (a ladder never straddles workgroups:
// LPB = (256 / G) / R ladders per block, the groups past LPB * R idle), possibly in different waves.
//
// A swap RELABELS, it does not move state: every walker carries the slot it currently represents.  At a swap event the
// walkers post their energies to an LDS table indexed [ladder in block][slot], both partners of a pair read the two energies
// and the pair's uniform and reach the same decision, and each changes its own slot.  Everything addressed in memory follows
// the SLOT -- the Philox element (c * R + slot) * dim + col, the injected draws, the trajectory (stored by whichever walker
// holds slot 0) and the final store to row c * R + slot -- through the addressing view A, a copy of L whose chain
// is the slot's row.  What is physical -- the lane's columns, its place in the wave (the Gaussian exchange row) -- stays in
// the Lane L that Energy::init saw.
#pragma once
#include "rows.h"

namespace ebm {
namespace ladder {
using namespace rows;

// Host side: the energy table (one float per lane group) goes behind what plan_params laid out in dynamic LDS.  Returns the
// blocks of the launch.
inline int64_t plan(const Geometry& geo, int n_replicas, int64_t n_ladders, size_t& smem, int& table_offset_floats) {
  table_offset_floats = (int)(smem / sizeof(float));
  smem += (size_t)(kBlock / geo.G) * sizeof(float);
  return ceil_div64(n_ladders, (kBlock / geo.G) / n_replicas);
}

// Where the draws of a swap event come from: the injected uniforms [n_events, n_rows], or (u == nullptr) Philox at the
// counter the kernel names for this event.
struct SwapDraws {
  const float* u;
  RngKey key;
  uint64_t counter;
};

// Who a lane group is: its ladder, its first slot, and where the ladder's rows start.
struct Place {
  int lpb, lib, slot;  // ladders per block, ladder in block, the slot the walker represents at the start
  int64_t ladder, row_base;
};

// Fills the physical lane L of a walker -- columns, lane-in-group and place in the wave by the thread id, chain and active
// flag by the ladder -- and says where it stands.  L.valid is still Lane::init's: the kernel rebuilds it for L.active.
template <class LaneT>
__device__ __forceinline__ Place place_walker(LaneT& L, int R, int dim, int64_t n_ladders) {
  constexpr int G = LaneT::G;
  Place w;
  w.lpb = (kBlock / G) / R;
  const int walker = (int)threadIdx.x / G;  // lane group in the block
  w.lib = walker / R;
  w.ladder = (int64_t)blockIdx.x * w.lpb + w.lib;
  w.slot = walker - w.lib * R;
  L.init(0, dim);  // the chain comes from the ladder, not the thread id
  L.active = w.lib < w.lpb && w.ladder < n_ladders;
  w.row_base = L.active ? w.ladder * (int64_t)R : 0;
  L.chain = w.row_base + w.slot;
  return w;
}

// One swap event.  The walker posts `e_now` (the energy of the state it holds) to e_table [kBlock / G], indexed
// lib * R + slot; slot s pairs with s + 1 when s has the event's parity, with s - 1 otherwise (the ends may be unpaired);
// the pair (lo, lo + 1) swaps when u < exp(min(0, (beta[lo] - beta[lo + 1]) (E_lo - E_hi))), u the uniform of row
// row_base + lo.  swap_counts (or null): attempts of pair (p, p + 1) at p, accepts at R - 1 + p.
// Returns whether the slot changed (then `slot` and the addressing view's chain `row` follow; the caller reloads what it keeps
// per slot).  Counts the event.  Both barriers are in here: EVERY thread of the block has to arrive.
template <class LaneT>
__device__ __forceinline__ bool swap_event(const LaneT& L, const Place& w, int R, int64_t n_rows, int& event, int& slot, int64_t& row,
                                           float* e_table, float e_now, const float* beta, const SwapDraws& d, uint32_t* swap_counts) {
  const int lib = w.lib;
  if (L.lg == 0 && lib < w.lpb) e_table[lib * R + slot] = e_now;
  __syncthreads();
  const int parity = event & 1;
  const bool lower = ((slot - parity) & 1) == 0;
  const int lo = lower ? slot : slot - 1;
  const bool paired = L.active && lo >= parity && lo + 1 < R;
  bool swap = false;
  if (paired) {
    const float e_lo = e_table[lib * R + lo], e_hi = e_table[lib * R + lo + 1];
    const float delta = (beta[lo] - beta[lo + 1]) * (e_lo - e_hi);
    const int64_t urow = w.row_base + lo;
    float uu;
    if (d.u) uu = d.u[(int64_t)event * n_rows + urow];
    else uu = u01_half_open(pick(philox_at(d.key, (uint64_t)urow >> 2, d.counter), (int)(urow & 3)));
    swap = delta == delta && uu < expf(fminf(delta, 0.0f));
  }
  if (swap_counts) {  // one ballot and one atomic per wave and pair, counted by the leader lane of the lower slot's walker
    const bool counts = paired && lower && L.lg == 0;
    for (int p = parity; p + 1 < R; p += 2) {
      const unsigned long long tried = __ballot(counts && lo == p);
      if (tried == 0ull) continue;
      const unsigned long long took = __ballot(counts && lo == p && swap);
      if ((threadIdx.x & 63) == 0) {
        atomicAdd(swap_counts + p, (uint32_t)__popcll(tried));
        if (took) atomicAdd(swap_counts + (R - 1) + p, (uint32_t)__popcll(took));
      }
    }
  }
  __syncthreads();  // the table is read: the next event may overwrite it
  if (swap) {
    slot = lower ? slot + 1 : slot - 1;
    row = w.row_base + slot;
  }
  ++event;
  return swap;
}

}  // namespace ladder
}  // namespace ebm
