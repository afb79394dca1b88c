// Kernel body of replica-exchange HMC on the wide MLP energy (ebm_tempering_hmc_mlp_chain_f32, include/ebm_hip.h;
// docs/design/tempering_hmc_mlp.md): the slot's draw, the accept, the swap event and the counters put around the shared leapfrog
// state machine (mlp_wide_leapfrog.inc, with the plain gradient and H0 = E + K as its hooks) and through it around the one
// evaluation (mlp_wide_setup.inc, mlp_wide_eval.inc); rows, noise and the launch are mlp_wide_rows.h's.  Two translation units
// instantiate it (compiled in parallel): mlp_wide_tempering.hip (H = 64) and mlp_wide_tempering_h128.hip (H = 128).
//
// One wave is 32 consecutive rows of the slot matrix [n_ladders * R, dim], R in {2, 4, 8, 16, 32}: 32 / R whole ladders.  A lane's
// slot is m & (R - 1) for the whole call and its partner at an event is the lane m +- 1 of the same K-half, so an event needs no
// LDS and no barrier.  A walker keeps its ROW: a swap moves the STATES, 16 DT position registers exchanged with the partner lane
// by a cross-lane read, and a lane that swapped stores its new row -- a lane reads back only what it stored itself.
//
// The held x lives in a.x between transitions.  A transition is n_leapfrog + 1 evaluations and carries no energy, force or
// momentum to the next one, so the bits do not depend on where a run is cut (up to the parity of the events, which restarts with
// every call).  An event evaluates nothing: E0 and E1 are both live at the decision and the energy of the state a slot now holds
// is accept ? E1 : E0.
//
// Counters: a lane counts its slot's accepted proposals and its pair's accepted swaps in two registers; the attempts follow from
// the number of events.  At the end of the call the waves add them up by slot across their lanes, the workgroup adds the waves'
// sums in LDS -- the first 3 R words of the weights' area, dead by then, between barriers every wave reaches -- and R threads
// flush them with one global atomic per address and workgroup.  No LDS is added, so the offsets of mlp_wide_setup.inc stand.
#pragma once
#include "mlp_wide_rows.h"

namespace ebm {
namespace widemlp {

struct WideTemperArgs {
  float* x;                 // [n_chains, dim], n_chains = n_ladders * R: the slot matrix, in/out
  int64_t n_chains;
  int32_t R, dim, n_mh, n_leapfrog, swap_every, thin, n_kept;
  const float* eps;         // device [R]
  const float* sqrt_temp;   // device [R]
  const float* beta;        // device [R]
  float* traj;              // [n_ladders, n_kept, dim] or null
  uint8_t* accept_mask;     // [n_mh, n_chains] or null
  uint32_t* accept_counts;  // [R] or null
  uint32_t* swap_counts;    // [2 (R - 1)]: attempts of pair (p, p + 1) at p, accepts at R - 1 + p; or null
  const float* p_noise;     // [n_mh, n_chains, dim] or null
  const float* u_accept;    // [n_mh, n_chains] or null
  const float* u_swap;      // [n_events, n_chains] or null
  RngKey key;
  uint64_t step0;
  const float* params;
  const char* w1_image;  // always null: the shared set-up text names it for MODE 3, which this kernel is not built for
};

template <int HT, int DT, int MODE>
__global__ __launch_bounds__(kBlock, 1) void mlp_wide_tempering_chain(WideTemperArgs a) {
  static_assert(MODE == 0 || MODE == 2, "weights in LDS: fp32 (0) or split bf16 images (2)");
  constexpr bool EVAL_SCALED = false;
#include "mlp_wide_setup.inc"
  EBM_WIDE_WALKS_ONCE_OPAQUE();  // (mlp_wide_rows.h)

  const int R = a.R, log2_r = __builtin_ctz((unsigned)a.R);  // wave-uniform
  uint32_t n_accepted = 0u, n_swapped = 0u;  // of this lane's slot; of the pair whose lower slot it is (counted where h == 0)
  int kept = 0, until_keep = a.thin, until_swap = a.swap_every, event = 0;
  for (int t = 0; t < a.n_mh; ++t) {  // wave-uniform
    EBM_WIDE_STEP_COPIES_OPAQUE();  // smp, hq, key (mlp_wide_rows.h): the slot and its constants are formed here.
    const Lanes lanes_t{dim, quads, active, hq};  // (the helpers see the opaque K-half)
    const int slot = (int)smp & (R - 1);
    const float eps = a.eps[slot], half_eps = 0.5f * eps, sqrt_temp = a.sqrt_temp[slot], beta = a.beta[slot];

    // ---- the velocity draw w = sqrt_temp z, a register quad at a time
    float p[DT][16];
    {
      const float* noise_t = a.p_noise ? a.p_noise + (int64_t)t * a.n_chains * dim : nullptr;
#pragma unroll
      for (int td = 0; td < DT; ++td)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int c0 = 32 * td + 8 * q + 4 * hq;
          EBM_WIDE_NOISE_QUAD(z, noise_t, lanes_t, a.step0 + 3ull * (uint64_t)t);  // (mlp_wide_rows.h)
#pragma unroll
          for (int j = 0; j < 4; ++j) p[td][4 * q + j] = (c0 + j < dim) ? sqrt_temp * z[j] : 0.0f;
        }
    }

    float xr[DT][16];
    load_rows(lanes_t, xr, a.x, smp);
    float e0 = 0.0f;  // E at the held state: what the slot holds after a reject
    const auto leapfrog_grad = [&](int, int, float gr) __attribute__((always_inline)) { return gr; };
    const auto leapfrog_held = [&](float energy) __attribute__((always_inline)) {
      e0 = energy;
      return clamp_nanprop(energy, -1e10f, 1e10f) + kinetic_plain<DT>(p);
    };
#include "mlp_wide_leapfrog.inc"
    // E at the proposal: xr is the position e_last was evaluated at on either path
    const float h1 = clamp_nanprop(e_last, -1e10f, 1e10f) + kinetic_plain<DT>(p);

    // ---- Metropolis accept at the slot's temperature: the Hamiltonian of exp(-E / T) with w ~ N(0, T) is beta (E + K(w))
    const float dlt = clamp_nanprop(beta * (h0 - h1), -50.0f, 50.0f);
    float acc_p = expf(dlt);
    acc_p = (acc_p > 1.0f) ? 1.0f : acc_p;  // NaN stays NaN and rejects
    float uu;
    if (a.u_accept) uu = active ? a.u_accept[(int64_t)t * a.n_chains + smp] : 2.0f;
    else uu = u01_half_open(pick(philox_at(key, (uint64_t)smp >> 2, a.step0 + 3ull * (uint64_t)t + 1ull), (int)(smp & 3)));
    const bool accept = active && (uu < acc_p);
    if (accept) store_rows(lanes_t, a.x, smp, xr);
    if (a.accept_mask && active && hq == 0) a.accept_mask[(int64_t)t * a.n_chains + smp] = accept ? 1 : 0;
    n_accepted += (accept && hq == 0) ? 1u : 0u;

    const bool event_now = --until_swap == 0;                                  // wave-uniform: (t + 1) % swap_every == 0
    const bool keep_now = --until_keep == 0;                                   // ... (t + 1) % thin == 0
    const bool store_kept = keep_now && a.traj != nullptr && kept < a.n_kept;  // ...
    if ((event_now || store_kept) && !accept) {
      // the held position stayed: the lane's own row (through an opaque copy of the pointer: forwarded from the load in front of
      // the trajectory, the plane would live in registers through every evaluation)
      const float* x_plane = a.x;
      asm volatile("" : "+s"(x_plane));
      load_rows(lanes_t, xr, x_plane, smp);
    }

    if (event_now) {
      until_swap = a.swap_every;
      // ---- the swap event (EBM_WIDE_SWAP_DECISION, mlp_wide_rows.h: lower, partner, swap), on the energy of the state the slot
      // now holds
      const float e_now = accept ? e_last : e0;
      EBM_WIDE_SWAP_DECISION(e_now, a.u_swap, a.step0 + 3ull * (uint64_t)t + 2ull);
      if (__any(swap)) {  // wave-uniform: every lane takes part in the cross-lane reads
#pragma unroll
        for (int td = 0; td < DT; ++td)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float other = __shfl(xr[td][r], partner);
            xr[td][r] = swap ? other : xr[td][r];
          }
        if (swap) store_rows(lanes_t, a.x, smp, xr);
      }
      n_swapped += (swap && lower && hq == 0) ? 1u : 0u;
      ++event;
    }

    if (keep_now) {
      until_keep = a.thin;
      if (store_kept && active && slot == 0) store_rows(lanes_t, a.traj, (smp >> log2_r) * (int64_t)a.n_kept + kept, xr);
      ++kept;
    }
  }

  if (a.accept_counts || a.swap_counts) {  // wave-uniform; every wave of the workgroup ran the same n_mh transitions
    // by slot across the wave: the lanes m, m + R, m + 2 R, .. of the K-half 0 hold one slot (the K-half 1 counted nothing)
    for (int d = R; d < 32; d <<= 1) {
      n_accepted += __shfl_xor(n_accepted, d);
      n_swapped += __shfl_xor(n_swapped, d);
    }
    uint32_t* table = reinterpret_cast<uint32_t*>(wide_smem);  // [R] accepts, [R] swaps taken, [R] pairs that tried: the weights are dead
    __syncthreads();
    if ((int)threadIdx.x < 3 * R) table[threadIdx.x] = 0u;
    __syncthreads();
    const int n_ladders_here = __popcll(__ballot(active && h == 0)) >> log2_r;  // (the wave's rows are whole ladders)
    if (lane < R) {  // (lane == slot here)
      // the events a pair with the lower slot `lane` took part in: those of its parity
      const int my_events = (lane + 1 < R) ? ((lane & 1) ? event / 2 : (event + 1) / 2) : 0;
      if (n_accepted) atomicAdd(&table[lane], n_accepted);
      if (n_swapped) atomicAdd(&table[R + lane], n_swapped);
      if (my_events && n_ladders_here) atomicAdd(&table[2 * R + lane], (uint32_t)(my_events * n_ladders_here));
    }
    __syncthreads();
    if ((int)threadIdx.x < R) {
      const int s = threadIdx.x;
      if (a.accept_counts && table[s]) atomicAdd(a.accept_counts + s, table[s]);
      if (a.swap_counts && s + 1 < R) {
        if (table[2 * R + s]) atomicAdd(a.swap_counts + s, table[2 * R + s]);
        if (table[R + s]) atomicAdd(a.swap_counts + (R - 1) + s, table[R + s]);
      }
    }
  }
}

struct TemperWalk {  // (launch_walk_by_dim, mlp_wide_rows.h)
  template <int HT, int DT, int MODE>
  static constexpr auto kernel = &mlp_wide_tempering_chain<HT, DT, MODE>;
};

}  // namespace widemlp
}  // namespace ebm
