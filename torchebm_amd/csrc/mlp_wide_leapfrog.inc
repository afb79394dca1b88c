// The leapfrog trajectory of a Metropolis-corrected walk on the wide MLP energy, a state machine around the ONE evaluation site
// (mlp_wide_plain_eval.inc): n_leapfrog + 1 evaluations -- mode 0: E and dE/dx at the held state, mode 1: after a kick + drift,
// mode 2: re-evaluation on a scrubbed position, decided per wave.  Included by mlp_wide_ais_body.h and mlp_wide_ghmc_body.h
// inside their transition loops; mlp_wide_hmc_body.h spells the same machine itself.
// In scope: what mlp_wide_plain_eval.inc expects; DT; a.n_leapfrog; eps, half_eps; hq, the lane's K-half; the position xr[DT][16]
// and the momentum p[DT][16] in the C/D layout; and two always-inline lambdas:
//   leapfrog_grad(td, r, gr)  the raw gradient of the walked energy at register (td, r), from gr = g[td][r] of dE/dx
//   leapfrog_held(energy)     what the evaluation at the held state is for, from its E: returns the start Hamiltonian
// Defines h0 (the start Hamiltonian), e_last (E at the position xr holds when the loop ends: the proposal's, on either path) and
// f (the last clamped force); p is the proposal's momentum.
    float f[DT][16];
#pragma unroll
    for (int td = 0; td < DT; ++td)
#pragma unroll
      for (int r = 0; r < 16; ++r) f[td][r] = 0.0f;
    float h0 = 0.0f, e_last = 0.0f;
    int done = 0, mode = 0;  // wave-uniform
    while (done <= a.n_leapfrog) {
      if (mode == 1) {  // first half kick + drift
#pragma unroll
        for (int td = 0; td < DT; ++td)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float ph = __builtin_fmaf(half_eps, f[td][r], p[td][r]);
            p[td][r] = ph;
            const float xn = __builtin_fmaf(eps, ph, xr[td][r]);
            xr[td][r] = (32 * td + row_of(r, hq) < dim) ? xn : 0.0f;
          }
      }
      constexpr bool eval_need_energy = true;
#include "mlp_wide_plain_eval.inc"
      if (mode == 0) {  // the start Hamiltonian and the first (clamped) force, both from this evaluation at the held state
        h0 = leapfrog_held(energy);
#pragma unroll
        for (int td = 0; td < DT; ++td)
#pragma unroll
          for (int r = 0; r < 16; ++r) f[td][r] = clamp_nanprop(-leapfrog_grad(td, r, g[td][r]), -1e6f, 1e6f);
        e_last = energy;
        mode = 1;
        ++done;
      } else if (mode == 1) {
        // The gradient at the proposal's position (f is free between the kick above and the force below).  The fast path needs
        // energy and gradient finite in every chain of the wave (a finite E vouches for x, as in mlp_wide_hmc_body.h; with a
        // base term in the gradient, a finite gradient does wherever the base's weight is not zero); decided per WAVE because
        // the literal path re-runs the MFMA evaluation.
        float gz = 0.0f;
#pragma unroll
        for (int td = 0; td < DT; ++td)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float gm = leapfrog_grad(td, r, g[td][r]);
            f[td][r] = gm;
            gz = __builtin_fmaf(gm, 0.0f, gz);
          }
        const bool all_fine = (bool)__all((__builtin_fabsf(energy) < __builtin_inff()) && gz == 0.0f);
        if (all_fine) {
          float pz = 0.0f;
#pragma unroll
          for (int td = 0; td < DT; ++td)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const float fn = __builtin_amdgcn_fmed3f(-f[td][r], -1e6f, 1e6f);
              const float pn = __builtin_fmaf(half_eps, fn, p[td][r]);
              f[td][r] = fn;
              p[td][r] = pn;
              pz = __builtin_fmaf(pn, 0.0f, pz);
            }
          if (pz != pz) {  // momentum overflow: x is finite, so f stands
#pragma unroll
            for (int td = 0; td < DT; ++td)
#pragma unroll
              for (int r = 0; r < 16; ++r) p[td][r] = nan_to_num0(p[td][r]);
          }
          e_last = energy;
          ++done;
        } else {  // literal semantics: NaN-propagating clamp, scrub, then re-evaluate on the scrubbed x
#pragma unroll
          for (int td = 0; td < DT; ++td)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const float fn = clamp_nanprop(-f[td][r], -1e6f, 1e6f);
              p[td][r] = nan_to_num0(__builtin_fmaf(half_eps, fn, p[td][r]));
              xr[td][r] = nan_to_num0(xr[td][r]);
            }
          mode = 2;
        }
      } else {  // mode 2: force and energy on the scrubbed position
#pragma unroll
        for (int td = 0; td < DT; ++td)
#pragma unroll
          for (int r = 0; r < 16; ++r) f[td][r] = clamp_nanprop(-leapfrog_grad(td, r, g[td][r]), -1e6f, 1e6f);
        e_last = energy;
        mode = 1;
        ++done;
      }
    }
