// Kernel body of the three-hidden-layer SiLU MLP energy (EBM_ENERGY_MLP3, include/ebm_hip_mlp3.h; docs/design/mlp3.md):
//     E(x) = w4 . silu(W3 silu(W2 silu(W1 x + b1) + b2) + b3) + b4
// One template <HT, DT> serves the Langevin chain (k_steps > 0) and the evaluation-only launch (k_steps == 0).  The lane
// geometry is the two-layer kernels': a wave owns 32 chains, a workgroup is four waves, everything is transposed (rows =
// feature, columns = chain) in the 32x32 MFMA C/D layout -- register r of one result is the B operand of the next contraction,
// and dE/dx comes out where the state lives.  Rows, noise, the update and the lane helpers are mlp_wide_rows.h's; the matrix
// operands are mlp_b16.h's (H = 64: three split bf16 images per matrix, all resident) or mlp_wide_body.h's contract<> on fp32
// words (H = 128: two H x H split images do not fit LDS together, so this width runs the exact-f32 matrix instruction).
// The set-up (parameters, LDS carve-up, staging, lane geometry) is mlp3_setup.inc, shared with mlp3_hmc_body.h.
// The evaluation is text of its own, mlp3_eval.inc: six contractions and five epilogues, in order, nothing hidden behind
// anything.  Two translation units instantiate the kernel: mlp3.hip (H = 64, DT 1 / 2 / 4) and mlp3_h128.hip (H = 128, DT 1).
#pragma once
#include "mlp_wide_rows.h"

namespace ebm {
namespace mlp3 {

using namespace widemlp;  // kBlock, f32x16, row_of, sigmoid_fast, contract<>, Lanes, load_rows, store_rows, normal_quad, wide_smem

struct Args {
  const float* x_src;  // [n, dim]: the start state (chain) or the points (evaluation); may be x itself
  float* x;            // [n, dim]: the chain's output (k_steps > 0)
  int64_t n_chains;
  int32_t dim, k_steps;
  float eta, sqrt_eta, noise_coef;
  const float* noise;  // [k, n, dim] or null
  RngKey key;
  uint64_t step0;
  const float* params;  // packed W1[H,dim] b1[H] W2[H,H] b2[H] W3[H,H] b3[H] w4[H] b4[1]
  float* energy_out;    // k_steps == 0: E(x)[n] or null
  float* grad_out;      // k_steps == 0: dE/dx[n, dim] or null (null: the forward pass only)
};

// LDS, H = 64:  [b1 b2 b3 w4][W2 image][W3 image][W1 image]                  1 KB + 24 KB + 24 KB + 12 / 24 / 48 KB
//      H = 128: [W2: H x (H + 1)][W3: H x (H + 1)][W1: H x (DP + 1)][b1 b2 b3 w4]   66 KB + 66 KB + 16.5 KB + 2 KB (DT = 1)
__host__ __device__ constexpr size_t smem_bytes(int ht, int dt) {
  const int H = 32 * ht, DP = 32 * dt;
  return ht == 2 ? (size_t)4 * H * sizeof(float) + 2 * mlpb16::image_bytes(H, H) + mlpb16::image_bytes(H, b16_cols(dt))
                 : (size_t)(2 * H * (H + 1) + H * (DP + 1) + 4 * H) * sizeof(float);
}

template <int HT, int DT>
__global__ __launch_bounds__(kBlock, 1) void mlp3_chain(Args a) {
  static_assert(HT == 2 || HT == 4, "hidden width 64 (split bf16 images) or 128 (fp32 words)");
  constexpr bool B16 = HT == 2;
  constexpr int H = 32 * HT, DP = 32 * DT;
  constexpr int C1 = b16_cols(DT);        // B16: width of the W1 image
  constexpr int S1 = DP + 1, S2 = H + 1;  // fp32 words: the conflict-free row strides
#include "mlp3_setup.inc"
  EBM_WIDE_LANES();

  // the state in the C/D layout: xr[td][r] = x[sample][32 td + row_of(r, h)], exactly zero beyond dim
  float xr[DT][16];
  load_rows(lanes, xr, a.x_src, sample);
  const float eta = a.eta, sqrt_eta = a.sqrt_eta, noise_coef = a.noise_coef;
  const bool forward_only = a.k_steps == 0 && !a.grad_out;  // wave-uniform
  const int n_evals = a.k_steps > 0 ? a.k_steps : 1;

  for (int step = 0; step < n_evals; ++step) {
    EBM_WIDE_STEP_COPIES_OPAQUE();  // smp, hq, key: nothing derived from them is hoisted out of the loop
    const Lanes lanes_q{dim, quads, active, hq};
#include "mlp3_eval.inc"
    if (a.k_steps == 0) {  // evaluation only
      if (active) {
        if (a.energy_out && hq == 0) a.energy_out[smp] = energy;
        if (a.grad_out) {
          float gr[DT][16];
#pragma unroll
          for (int td = 0; td < DT; ++td)
#pragma unroll
            for (int r = 0; r < 16; ++r) gr[td][r] = g[td][r];
          store_rows(lanes_q, a.grad_out, smp, gr);
        }
      }
      return;
    }
    // ---- Euler-Maruyama, the reference's order, a register quad at a time (mlp_wide_rows.h)
    const float* noise_i = a.noise ? a.noise + (int64_t)step * a.n_chains * dim : nullptr;
#pragma unroll
    for (int td = 0; td < DT; ++td)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c0 = 32 * td + 8 * q + 4 * hq;
        EBM_WIDE_NOISE_QUAD(z, noise_i, lanes_q, a.step0 + (uint64_t)step);
        EBM_WIDE_EULER_MARUYAMA_QUAD();
      }
  }
  if (active) store_rows(lanes, a.x, sample, xr);
}

// One launch of KERNEL, a kernel of this energy at (HT, DT) that takes its arguments by value: the per-device LDS opt-in, one wave
// per 32 chains.
template <auto KERNEL, int HT, int DT, class KernelArgs>
int launch_kernel(const KernelArgs& a, hipStream_t st, const char* who) {
  constexpr size_t smem = smem_bytes(HT, DT);
  static_assert(smem <= 160 * 1024, "the weights of this shape do not fit the CU's LDS");
  static DeviceOnce attr_once;  // the LDS opt-in is a per-device function attribute
  if (attr_once.first())        // > 64 KiB of dynamic LDS needs the opt-in
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  const int64_t blocks = ceil_div64(a.n_chains, 32 * (kBlock / 64));
  if (blocks > 0x7fffffffLL) return fail(EBM_EINVAL, "%s: too many chains for one launch", who);
  hipLaunchKernelGGL(KERNEL, dim3((unsigned)blocks), dim3(kBlock), smem, st, a);
  return check_launch(who);
}

template <int HT, int DT>
int launch(const Args& a, hipStream_t st, const char* who) {
  return launch_kernel<&mlp3_chain<HT, DT>, HT, DT>(a, st, who);
}

int launch_h128(const Args& a, hipStream_t st, const char* who);  // mlp3_h128.hip

}  // namespace mlp3
}  // namespace ebm
