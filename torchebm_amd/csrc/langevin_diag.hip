// Element-wise Langevin chain kernels that also emit the per-block diagnostics records (diag.h) at the kept
// steps: the DIAG instantiations of the lean k-fused kernel, in their own translation unit so that they
// compile beside langevin.hip.  Reference: torchebm/samplers/langevin_dynamics.py:170-185.
#include "langevin_elem.h"

namespace ebm {

// Block geometry of the flat kernel: 256 lanes x one float4 = 1024 consecutive elements per workgroup.
bool elem_diag_supported(int32_t dim, bool has_noise, bool has_traj) {
  if (has_noise) return false;                       // the lean loop draws its own noise
  if (has_traj && (dim & 3) != 0) return false;      // float4 trajectory rows
  return (kBlock * 4) % dim == 0 || dim % (kBlock * 4) == 0;
}

bool elem_diag_plan(int64_t n_chains, int32_t dim, diag::DiagArgs& d) { return diag::plan(n_chains, dim, kBlock * 4, d); }

template <bool C64>
static int launch_diag(const LangevinChainReq& q, const ChainArgs& a, dim3 grid, dim3 block, size_t smem, hipStream_t st) {
#define EBM_D_T(KIND, TB, CL, HE)                                                                                             \
  do {                                                                                                                        \
    if (q.traj) hipLaunchKernelGGL((langevin_chain_lean_diag_kernel<KIND, TB, CL, true, HE, C64>), grid, block, smem, st, a); \
    else hipLaunchKernelGGL((langevin_chain_lean_diag_kernel<KIND, TB, CL, false, HE, C64>), grid, block, smem, st, a);       \
  } while (0)
#define EBM_D_H(KIND, HE)                                       \
  do {                                                          \
    if (q.coef_table && q.clamp) EBM_D_T(KIND, true, true, HE); \
    else if (q.coef_table) EBM_D_T(KIND, true, false, HE);      \
    else if (q.clamp) EBM_D_T(KIND, false, true, HE);           \
    else EBM_D_T(KIND, false, false, HE);                       \
  } while (0)
#define EBM_D(KIND)                  \
  do {                               \
    if (q.heun) EBM_D_H(KIND, true); \
    else EBM_D_H(KIND, false);       \
  } while (0)
  if (q.e.kind == EBM_ENERGY_DOUBLE_WELL) EBM_D(EBM_ENERGY_DOUBLE_WELL);
  else EBM_D(EBM_ENERGY_HARMONIC);
#undef EBM_D
#undef EBM_D_H
#undef EBM_D_T
  return check_launch(q.heun ? "ebm_langevin_heun_chain_f32" : "ebm_langevin_chain_f32");
}

int launch_langevin_chain_elem_diag(const LangevinChainReq& q, hipStream_t st) {
  const char* who = q.heun ? "ebm_langevin_heun_chain_f32" : "ebm_langevin_chain_f32";
  const int32_t dim = q.dim;
  ChainArgs a = elem_chain_args(q);
  if (!elem_diag_plan(q.n_chains, dim, a.diag)) return fail(EBM_EDIM, "%s: diagnostics records need dim | 1024 or 1024 | dim on the flat kernel (dim %d)", who, dim);
  a.diag.partials = q.diag_partials;
  if (a.diag.n_blocks > 0x7fffffffLL) return fail(EBM_EINVAL, "%s: state too large for one launch", who);
  const dim3 grid((unsigned)a.diag.n_blocks), block(kBlock);
  const int lds_generic = diag::lds_floats(a.diag.E, a.diag.S), lds_fast = 2 * diag::fast_lds_floats();
  const size_t smem = (size_t)(diag::fast_flat_ok(dim) ? lds_fast : lds_generic) * sizeof(float);
  return lean_counters32(a) ? launch_diag<false>(q, a, grid, block, smem, st) : launch_diag<true>(q, a, grid, block, smem, st);
}

}  // namespace ebm
