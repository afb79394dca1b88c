// The folded DoubleWell loop on plain f32 instructions (langevin_elem.h lean_body PLAIN, kind 17): bench.py's headline kernel.
// The same operations in the same order as kind 16 (langevin.hip), one element per instruction where kind 16 issues
// v_pk_mul_f32 / v_pk_add_f32 on pairs: 88 vector instructions per float4 group and step against 70, and faster -- on this loop a
// packed-f32 instruction costs more issue time than the two plain ones it replaces (docs/design/langevin_flat.md,
// profiles/plain_fold_*).  A unit of its own because the Makefile compiles it with -fno-slp-vectorize: the SLP vectoriser
// would pack the element-wise code again.
#include "langevin_elem.h"

namespace ebm {

int langevin_lean_fold_plain_launch(const LangevinChainReq& q, float fold_eta, bool c64, unsigned blocks, hipStream_t st) {
  ChainArgs a = elem_chain_args(q);
  a.noise = nullptr;
  a.diag = diag::DiagArgs{nullptr, 0, 0, 0};
  a.fold_eta = fold_eta;
  const dim3 grid(blocks), block(kBlock);
  if (c64) hipLaunchKernelGGL((langevin_chain_lean_kernel<kDoubleWellFoldPlain, false, false, false, false, true>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((langevin_chain_lean_kernel<kDoubleWellFoldPlain, false, false, false, false, false>), grid, block, 0, st, a);
  return check_launch("ebm_langevin_chain_f32");
}

}  // namespace ebm
