// Kernel body of replica-exchange Langevin on the wide MLP energy (ebm_tempering_mlp_chain_f32, include/ebm_hip.h;
// docs/design/tempering_mlp.md): the Euler-Maruyama walk of mlp_wide_langevin_moments_body.h -- ONE evaluation site, the raw
// gradient, every operation of the update rounded on its own -- at the slot's noise_coef, with the swap event and the counters of
// mlp_wide_tempering_body.h between the evaluation and the step.  Two translation units instantiate it (compiled in parallel):
// mlp_wide_tempering_langevin.hip (H = 64) and mlp_wide_tempering_langevin_h128.hip (H = 128).
//
// One wave is 32 consecutive rows of the slot matrix [n_ladders * R, dim], R in {2, 4, 8, 16, 32}: 32 / R whole ladders.  A lane's
// slot is m & (R - 1) for the whole call and its partner at an event is the lane m +- 1 of the same K-half, so an event needs no
// LDS and no barrier.  A walker keeps its ROW: a swap moves the STATE.
//
// An event costs no evaluation.  Iteration i evaluates (E, g) at the state behind step i - 1; the event due behind that step
// decides on these energies, and where any pair of the wave swaps, the 16 DT registers of x AND the 16 DT registers of g are
// taken from the partner lane by cross-lane reads: the gradient was evaluated at the state and moves with it, so step i starts
// from the pair (x, g) the event left.  x lives in registers from the one load_rows to the one store_rows; nothing reaches memory
// at an event.  A call makes k_steps + 1 evaluations when an event is due behind the last step (the last one for its energies
// alone) and k_steps otherwise: a kept step behind the last step with no event due there stores slot 0's row as it stands and
// evaluates nothing.
//
// Counters: a lane counts its pair's accepted swaps in one register (the lower slot's lane, K-half 0); the attempts follow from
// the number of events.  At the end of the call the waves add them up by slot across their lanes, the workgroup adds the waves'
// sums in LDS -- the first 2 R words of the weights' area, dead by then, between barriers every wave reaches -- and R - 1 threads
// flush them with one global atomic per non-zero address and workgroup.  No LDS is added, so the offsets of mlp_wide_setup.inc stand.
#pragma once
#include "mlp_wide_rows.h"

namespace ebm {
namespace widemlp {

struct WideTemperLangevinArgs {
  float* x;                 // [n_chains, dim], n_chains = n_ladders * R: the slot matrix, in/out
  int64_t n_chains;
  int32_t R, dim, k_steps, swap_every, thin, n_kept;
  float eta, sqrt_eta;
  const float* noise_coef;  // device [R]
  const float* beta;        // device [R]
  float* traj;              // [n_ladders, n_kept, dim] or null
  uint32_t* swap_counts;    // [2 (R - 1)]: attempts of pair (p, p + 1) at p, accepts at R - 1 + p; or null
  const float* noise;       // [k_steps, n_chains, dim] or null
  const float* u;           // [n_events, n_chains] or null
  RngKey key;
  uint64_t step0;
  const float* params;
  const char* w1_image;  // always null: the shared set-up text names it for MODE 3, which this kernel is not built for
};

template <int HT, int DT, int MODE>
__global__ __launch_bounds__(kBlock, 1) void mlp_wide_tempering_langevin_chain(WideTemperLangevinArgs a) {
  static_assert(MODE == 0 || MODE == 2, "weights in LDS: fp32 (0) or split bf16 images (2)");
  constexpr bool EVAL_SCALED = false;
#include "mlp_wide_setup.inc"
  EBM_WIDE_WALKS_ONCE_OPAQUE();  // (mlp_wide_rows.h)
  EBM_WIDE_LANES();

  const float eta = a.eta, sqrt_eta = a.sqrt_eta;
  const int R = a.R, log2_r = __builtin_ctz((unsigned)a.R);  // wave-uniform
  uint32_t n_swapped = 0u;  // of the pair whose lower slot this lane holds (counted where h == 0)
  int kept = 0, until_keep = a.thin, until_swap = a.swap_every, event = 0;
  float xr[DT][16];
  load_rows(lanes, xr, a.x, sample);

  for (int i = 0;; ++i) {  // wave-uniform
    // what is due behind step i - 1
    bool event_now = false, keep_now = false;
    if (i > 0) {
      event_now = --until_swap == 0;  // i % swap_every == 0
      keep_now = --until_keep == 0;   // i % thin == 0
      if (event_now) until_swap = a.swap_every;
      if (keep_now) until_keep = a.thin;
    }
    const bool store_kept = keep_now && a.traj != nullptr && kept < a.n_kept;
    if (i == a.k_steps && !event_now) {
      // nothing is evaluated behind the last step when no event is due there: a kept state goes out as it stands
      if (store_kept && active && ((int)sample & (R - 1)) == 0)
        store_rows(lanes, a.traj, (sample >> log2_r) * (int64_t)a.n_kept + kept, xr);
      break;
    }
    EBM_WIDE_STEP_COPIES_OPAQUE();  // smp, hq, key (mlp_wide_rows.h): the slot and its constant are formed here.
    const Lanes lanes_i{dim, quads, active, hq};  // (the helpers see the opaque K-half)
    const int slot = (int)smp & (R - 1);
    constexpr bool eval_need_energy = true;
#include "mlp_wide_plain_eval.inc"
    // the raw gradient and the unclamped energy of the state behind step i - 1 (no clamp: a NaN stays in its ladder)

    if (event_now) {
      // ---- the swap event behind step i - 1 (EBM_WIDE_SWAP_DECISION, mlp_wide_rows.h: lower, partner, swap)
      EBM_WIDE_SWAP_DECISION(energy, a.u, a.step0 + 2ull * (uint64_t)i - 1ull);
      if (__any(swap)) {  // wave-uniform: every lane takes part in the cross-lane reads
#pragma unroll
        for (int td = 0; td < DT; ++td)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float x_other = __shfl(xr[td][r], partner);
            const float g_other = __shfl(g[td][r], partner);
            xr[td][r] = swap ? x_other : xr[td][r];
            g[td][r] = swap ? g_other : g[td][r];
          }
      }
      n_swapped += (swap && lower && hq == 0) ? 1u : 0u;
      ++event;
    }

    if (keep_now) {
      if (store_kept && active && slot == 0) store_rows(lanes_i, a.traj, (smp >> log2_r) * (int64_t)a.n_kept + kept, xr);
      ++kept;
    }
    if (i == a.k_steps) break;

    // step i: x1 = x - eta g;  dw = z sqrt_eta;  x' = x1 + noise_coef[slot] dw -- every operation rounded on its own, a register
    // quad at a time
    const float noise_coef = a.noise_coef[slot];
    const float* noise_i = a.noise ? a.noise + (int64_t)i * a.n_chains * dim : nullptr;
#pragma unroll
    for (int td = 0; td < DT; ++td)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c0 = 32 * td + 8 * q + 4 * hq;
        EBM_WIDE_NOISE_QUAD(z, noise_i, lanes_i, a.step0 + 2ull * (uint64_t)i);  // (mlp_wide_rows.h)
        EBM_WIDE_EULER_MARUYAMA_QUAD();
      }
  }
  if (active) store_rows(lanes, a.x, sample, xr);

  // (the flush is spelled out here and in mlp_wide_tempering_body.h: one text for the tables of 2 R and 3 R words changed this
  // kernel, docs/design/mlp_wide.md)
  if (a.swap_counts) {  // wave-uniform; every wave of the workgroup ran the same k_steps steps
    // by slot across the wave: the lanes m, m + R, m + 2 R, .. of the K-half 0 hold one slot (the K-half 1 counted nothing)
    for (int d = R; d < 32; d <<= 1) n_swapped += __shfl_xor(n_swapped, d);
    uint32_t* table = reinterpret_cast<uint32_t*>(wide_smem);  // [R] swaps taken, [R] pairs that tried: the weights are dead
    __syncthreads();
    if ((int)threadIdx.x < 2 * R) table[threadIdx.x] = 0u;
    __syncthreads();
    const int n_ladders_here = __popcll(__ballot(active && h == 0)) >> log2_r;  // (the wave's rows are whole ladders)
    if (lane < R) {  // (lane == slot here)
      // the events a pair with the lower slot `lane` took part in: those of its parity
      const int my_events = (lane + 1 < R) ? ((lane & 1) ? event / 2 : (event + 1) / 2) : 0;
      if (n_swapped) atomicAdd(&table[lane], n_swapped);
      if (my_events && n_ladders_here) atomicAdd(&table[R + lane], (uint32_t)(my_events * n_ladders_here));
    }
    __syncthreads();
    if ((int)threadIdx.x + 1 < R) {
      const int s = threadIdx.x;
      if (table[R + s]) atomicAdd(a.swap_counts + s, table[R + s]);
      if (table[s]) atomicAdd(a.swap_counts + (R - 1) + s, table[s]);
    }
  }
}

struct TemperLangevinWalk {  // (launch_walk_by_dim, mlp_wide_rows.h)
  template <int HT, int DT, int MODE>
  static constexpr auto kernel = &mlp_wide_tempering_langevin_chain<HT, DT, MODE>;
};

}  // namespace widemlp
}  // namespace ebm
