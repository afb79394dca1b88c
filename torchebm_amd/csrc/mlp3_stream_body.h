// The three-hidden-layer SiLU MLP energy at hidden width 128 on the bf16 matrix pipe, dim <= 128 (include/ebm_hip_mlp3_stream.h;
// docs/design/mlp3_stream.md).  mlp3_body.h's geometry, update, noise and rows, and the six contractions and five epilogues of
// mlp3_eval.inc's split-bf16 form (v_mfma_f32_32x32x16_bf16, six products per K-block, smallest first) -- but two split
// 128 x 128 images are 2 x 96 KB against the CU's 160 KB, so only W2 is resident.  W3 and W1 come from a PRE-SPLIT image in
// global memory (mlp3_build_image, mlp3_stream.hip) in PIECES of 24 576 bytes through two LDS buffers, filled by LDS-direct
// loads one piece ahead of the MFMAs (mlp_b16.h: slab_request / slab_wait):
//     W3: four slabs [32][128] x 3 splits -- one output tile of the forward walk, one K-block pair of the transposed walk;
//     W1: N1 = C1 / 32 pieces [4096 / C1][C1] x 3 splits (C1 = 32 / 64 / 128 for DT = 1 / 2 / 4) -- 4 / 2 / 1 output tiles of
//         the forward walk, 8 / 4 / 2 K-blocks of the transposed walk.
// One evaluation consumes the LOADS 0 .. 2 N1 + 6, load i in buffer i & 1:
//     W1 pieces 0 .. N1 - 1 | W3 slabs 0 1 2 3 | (slab 3 again) 2 1 0 | W1 pieces N1 - 1 .. 0
// The sequence is a palindrome of even length, so load i and load 2 N1 + 6 - i are the same piece in the same buffer, and a
// piece that is still there is not fetched again: slab 3 and then slab 2 of the transposed W3 walk are where the forward walk
// left them, and the last two loads of an evaluation are loads 1 and 0 of the next -- no request crosses from one evaluation to
// the next, so whether another one follows decides nothing.  A load that is fetched is requested when the load before it starts
// being consumed, behind that load's slab_wait(): its buffer held the load before that one, which every wave has left.  Loads
// 0 and 1 of the first evaluation are requested at the set-up.  2 N1 + 4 transfers per evaluation; every requested piece is
// awaited and consumed, so none is in flight when the workgroup ends (a forward-only launch ends behind W3's slab 3, the
// last one requested by then).
#pragma once
#include "mlp3_body.h"

namespace ebm {
namespace mlp3 {

// LDS: [b1 b2 b3 w4: 2 KB][buffer 0: 24 KB][buffer 1: 24 KB][W2 image: 96 KB] = 149 504 of 163 840 bytes
constexpr uint32_t kStreamVecBytes = 4u * 128u * (uint32_t)sizeof(float);
constexpr uint32_t kStreamBuf0 = kStreamVecBytes, kStreamBuf1 = kStreamBuf0 + mlpb16::kSlabBytes;
constexpr uint32_t kStreamImg2 = kStreamBuf1 + mlpb16::kSlabBytes;
constexpr size_t kStreamSmem = kStreamImg2 + mlpb16::image_bytes(128, 128);
static_assert(kStreamBuf1 + mlpb16::kSlabBytes <= 65536u, "slab_request puts a 16-bit LDS address into M0: both buffers below 64 KiB");
static_assert(kStreamSmem <= 160 * 1024, "the CU's LDS");

__host__ __device__ constexpr int stream_pieces(int c1) { return c1 / 32; }  // W1 pieces: 1 / 2 / 4
// piece of the global image [W1 pieces][W3 slabs] that load i of an evaluation is: a palindrome over 0 .. 2 n1 + 6
__host__ __device__ constexpr int stream_piece_of(int n1, int i) { return i < n1 + 4 ? i : 2 * n1 + 6 - i; }
// ... and whether an evaluation has to fetch it: not loads 0 and 1 (they are the last two loads of the evaluation before, or the
// set-up's), not load n1 + 4 (W3 slab 2, which load n1 + 2 left in the same buffer), and nothing behind the last load
__host__ __device__ constexpr bool stream_fetched(int n1, int i) { return i >= 2 && i != n1 + 4 && i <= 2 * n1 + 6; }

template <int DT>
__global__ __launch_bounds__(kBlock, 1) void mlp3_stream_chain(Args a, const char* __restrict__ image) {
  static_assert(DT == 1 || DT == 2 || DT == 4, "one, two or four state tiles");
  using namespace mlpb16;
  constexpr int HT = 4, H = 128;
  constexpr int C1 = b16_cols(DT), N1 = stream_pieces(C1), R1 = 4096 / C1, TP1 = R1 / 32;  // a W1 piece: R1 rows = TP1 tiles
  constexpr int NL = 2 * N1 + 6;  // the evaluation's last load
  static_assert(3 * R1 * C1 * 2 == (int)kSlabBytes, "a W1 piece is one buffer");
  const int dim = a.dim;
  const float* b1g = a.params + H * dim;
  const float* b2g = b1g + H + H * H;
  const float* b3g = b2g + H + H * H;
  const float* w4g = b3g + H;
  const float b4 = w4g[H];
  // ---- the LDS carve-up, the first two requests and the staging (once per launch)
  float* const b1s = wide_smem;
  float* const b2s = b1s + H;
  float* const b3s = b2s + H;
  float* const w4s = b3s + H;
  const lds_bytes lds0 = (lds_bytes)wide_smem;
  const int lane = threadIdx.x & 63;
  const Walk<R1, C1> p_walk0(lds0 + kStreamBuf0, lane), p_walk1(lds0 + kStreamBuf1, lane);                 // a W1 piece
  const Walk<kSlabRows, kSlabCols> s_walk0(lds0 + kStreamBuf0, lane), s_walk1(lds0 + kStreamBuf1, lane);  // a W3 slab
  const Walk<H, H> walk2(lds0 + kStreamImg2, lane);
  const uint32_t buf[2] = {p_walk0.base, p_walk1.base};
  static_assert(stream_piece_of(N1, NL) == 0 && stream_piece_of(N1, N1 + 3) == stream_piece_of(N1, N1 + 4) + 1, "the schedule above");
  slab_request(image, 0, buf[0], kBlock);  // loads 0 and 1 of the first evaluation
  slab_request(image, 1, buf[1], kBlock);
  stage_image<H, H>(b1g + H, H, H, lds0 + kStreamImg2, kBlock);
  for (int i = threadIdx.x; i < H; i += kBlock) {
    b1s[i] = b1g[i];
    b2s[i] = b2g[i];
    b3s[i] = b3g[i];
    w4s[i] = w4g[i];
  }
  __syncthreads();

  const int m = lane & 31, h = lane >> 5;
  const int64_t sample = ((int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * 32 + m;
  const bool active = sample < a.n_chains;  // chains past n are neither loaded nor stored
  const bool quads = (dim & 3) == 0;
  EBM_WIDE_LANES();

  // the state in the C/D layout: xr[td][r] = x[sample][32 td + row_of(r, h)], exactly zero beyond dim
  float xr[DT][16];
  load_rows(lanes, xr, a.x_src, sample);
  const float eta = a.eta, sqrt_eta = a.sqrt_eta, noise_coef = a.noise_coef;
  const bool forward_only = a.k_steps == 0 && !a.grad_out;  // workgroup-uniform
  const int n_evals = a.k_steps > 0 ? a.k_steps : 1;

  for (int step = 0; step < n_evals; ++step) {
    EBM_WIDE_STEP_COPIES_OPAQUE();  // smp, hq, key: nothing derived from them is hoisted out of the loop
    const Lanes lanes_q{dim, quads, active, hq};
    // Load i starts being consumed: it has landed for every wave, every wave has left the load before it, and the load behind
    // it is requested into that one's buffer -- unless the buffer holds that very piece already (see above).
    const auto begin_load = [&](auto ic) __attribute__((always_inline)) {
      constexpr int i = decltype(ic)::value;
      slab_wait();
      if constexpr (stream_fetched(N1, i + 1)) slab_request(image, stream_piece_of(N1, i + 1), buf[(i + 1) & 1], kBlock);
    };
    f32x16 g[DT];
    float energy;
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) g[t][r] = 0.0f;
#include "mlp3_b16_tiles.inc"
    f32x16 acc[HT];
    f32x2 s1[HT][8], s2[HT][8];
    Split8p spa[2 * HT], spb[2 * HT];  // the B operands, alternating: h1 | h2 | d3 | d2 | d1
    const auto w2 = walk2.opaque();   // (the image never changes: an opaque copy keeps the operand loads at their MFMAs)
    // ---- layer 1: loads 0 .. N1 - 1, W1 piece p = output tiles TP1 p .. TP1 p + TP1 - 1 over all 2 DT K-blocks
    bias_tiles(acc, b1s);
    static_for<N1>([&](auto pc) __attribute__((always_inline)) {
      constexpr int p = decltype(pc)::value;
      begin_load(pc);
      const auto ws = ((p & 1) ? p_walk1 : p_walk0).opaque();
      contract_pipe<TP1, 2 * DT, false, false>(
          reinterpret_cast<f32x16(&)[TP1]>(acc[TP1 * p]), ws,
          [&](auto kb) __attribute__((always_inline)) -> const Split8p& { return spx[decltype(kb)::value]; }, NoFill{});
    });
    static_for<HT>([&](auto tc) __attribute__((always_inline)) { silu_tile(tc, acc[decltype(tc)::value], s1[decltype(tc)::value], spa); });
    EBM_BLOCK_CUT();
    // ---- layer 2: the resident image, K = units of layer 1
    bias_tiles(acc, b2s);
    contract_pipe<HT, 2 * HT, false, false>(
        acc, w2, [&](auto kb) __attribute__((always_inline)) -> const Split8p& { return spa[decltype(kb)::value]; }, NoFill{});
    static_for<HT>([&](auto tc) __attribute__((always_inline)) { silu_tile(tc, acc[decltype(tc)::value], s2[decltype(tc)::value], spb); });
    EBM_BLOCK_CUT();
    // ---- layer 3: loads N1 .. N1 + 3, W3 slab t = output tile t over all eight K-blocks (two accumulators alternating);
    //      E += w4 silu(a3), d3 = w4 silu'(a3)
    bias_tiles(acc, b3s);
    static_for<HT>([&](auto tc) __attribute__((always_inline)) {
      constexpr int t = decltype(tc)::value, i = N1 + t;
      begin_load(std::integral_constant<int, i>{});
      const auto ws = ((i & 1) ? s_walk1 : s_walk0).opaque();
      contract_pipe<1, 2 * HT, false, false>(
          reinterpret_cast<f32x16(&)[1]>(acc[t]), ws,
          [&](auto kb) __attribute__((always_inline)) -> const Split8p& { return spb[decltype(kb)::value]; }, NoFill{});
    });
#include "mlp3_b16_energy.inc"
    EBM_BLOCK_CUT();
    if (!forward_only) {
      // ---- backward through W3: slab 3 is still resident, then loads N1 + 4 .. N1 + 6 = slabs 2 1 0; slab s = K-blocks
      //      2 s, 2 s + 1 of all four output tiles; d2 = (W3^T d3) s2
      zero_tiles(acc);
      static_for<HT>([&](auto kc) __attribute__((always_inline)) {
        constexpr int k = decltype(kc)::value, sl = HT - 1 - k, i = N1 + 3 + k;
        if constexpr (k > 0) begin_load(std::integral_constant<int, i>{});
        const auto ws = ((i & 1) ? s_walk1 : s_walk0).opaque();
        contract_pipe<HT, 2, false, true>(
            acc, ws, [&](auto kb) __attribute__((always_inline)) -> const Split8p& { return spa[2 * sl + decltype(kb)::value]; }, NoFill{});
      });
      static_for<HT>([&](auto tc) __attribute__((always_inline)) { back_tile(tc, acc[decltype(tc)::value], s2[decltype(tc)::value], spb); });
      EBM_BLOCK_CUT();
      // ---- backward through W2: K = units of layer 2; d1 = (W2^T d2) s1
      zero_tiles(acc);
      contract_pipe<HT, 2 * HT, false, true>(
          acc, w2, [&](auto kb) __attribute__((always_inline)) -> const Split8p& { return spb[decltype(kb)::value]; }, NoFill{});
      static_for<HT>([&](auto tc) __attribute__((always_inline)) { back_tile(tc, acc[decltype(tc)::value], s1[decltype(tc)::value], spa); });
      EBM_BLOCK_CUT();
      // ---- backward through W1: loads N1 + 7 .. 2 N1 + 6 = pieces N1 - 1 .. 0; piece p = K-blocks 2 TP1 p .. of all DT output
      //      tiles (image columns past dim are zero: the padding rows stay 0).  The last one stays for the next evaluation.
      static_for<N1>([&](auto kc) __attribute__((always_inline)) {
        constexpr int k = decltype(kc)::value, p = N1 - 1 - k, i = N1 + 7 + k;
        begin_load(std::integral_constant<int, i>{});
        const auto ws = ((i & 1) ? p_walk1 : p_walk0).opaque();
        contract_pipe<DT, 2 * TP1, false, true>(
            g, ws, [&](auto kb) __attribute__((always_inline)) -> const Split8p& { return spa[2 * TP1 * p + decltype(kb)::value]; }, NoFill{});
      });
    }
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
      break;
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
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (no transfer outlives its workgroup: none is left by construction)
  if (a.k_steps > 0 && active) store_rows(lanes, a.x, sample, xr);
}

template <int DT>
int launch_stream(const Args& a, const char* image, hipStream_t st, const char* who) {
  static DeviceOnce attr_once;  // the LDS opt-in is a per-device function attribute
  if (attr_once.first())        // > 64 KiB of dynamic LDS needs the opt-in
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(mlp3_stream_chain<DT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kStreamSmem);
  const int64_t blocks = ceil_div64(a.n_chains, 32 * (kBlock / 64));
  if (blocks > 0x7fffffffLL) return fail(EBM_EINVAL, "%s: too many chains for one launch", who);
  hipLaunchKernelGGL((mlp3_stream_chain<DT>), dim3((unsigned)blocks), dim3(kBlock), kStreamSmem, st, a, image);
  return check_launch(who);
}

}  // namespace mlp3
}  // namespace ebm
