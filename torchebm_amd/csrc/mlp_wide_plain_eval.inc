// The plain evaluation of the walks: mlp_wide_eval.inc with nothing stored, cut, pinned or hidden in its gaps.  In scope:
// what mlp_wide_eval.inc expects from the set-up, eval_need_energy (false where a walk never reads `energy`), and
// walk1_once / walk2_once (mlp_wide_rows.h: EBM_WIDE_WALKS_ONCE_*), which shadow the set-up's walks here.
      constexpr bool eval_energy_only = false, eval_block_cuts = false, eval_store_acts = false, eval_pin = false;
      [[maybe_unused]] float* const act_base = nullptr;
      [[maybe_unused]] constexpr uint32_t act_lane = 0;
      [[maybe_unused]] constexpr float act_seed = 1.0f;
      [[maybe_unused]] const auto eval_aux = [](auto) __attribute__((always_inline)) {};  // (nothing to hide in the tails' empty gaps)
      [[maybe_unused]] constexpr bool slab_more = true;  // MODE 3: every evaluation asks for the next one's first slab (drained at the end)
      const auto& walk1 = walk1_once;
      const auto& walk2 = walk2_once;
#include "mlp_wide_eval.inc"
