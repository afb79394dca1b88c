// One evaluation of the three-hidden-layer MLP energy (included by mlp3_body.h's kernel, once, inside its step loop).
// In scope: B16, HT, DT, H, S1, S2, the staged weights (walk1 / walk2 / walk3, or W1s / W2s / W3s), b1s, b2s, b3s, w4s, b4, m,
// hq (the lane's K-half, opaque per step), forward_only (wave-uniform: stop behind the forward pass) and the state xr[DT][16]
// in the C/D layout.  Defines g[DT] (dE/dx in the same layout; exactly zero in the padding rows) and `energy`.
//
// Six contractions -- W1 x, W2 h1, W3 h2, W3^T d3, W2^T d2, W1^T d1 -- with the K index of each enumerated in the order the
// C/D layout holds the previous result, so a result register is the next B operand as it stands:
//     a1 = W1 x + b1    h1 = silu(a1)    s1 = silu'(a1)
//     a2 = W2 h1 + b2   h2 = silu(a2)    s2 = silu'(a2)
//     a3 = W3 h2 + b3   E = w4 . silu(a3) + b4          d3 = w4 * silu'(a3)
//     d2 = (W3^T d3) * s2     d1 = (W2^T d2) * s1       dE/dx = W1^T d1
// The biases are the initial accumulators.  s1 and s2 stay in registers across the layers behind them (16 HT values each).
    f32x16 g[DT];
    float energy;
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) g[t][r] = 0.0f;
    if constexpr (B16) {
      // ------------------------------------------------------------------------------------------------------------------
      // H = 64: the bf16 matrix pipe with three-way split operands (mlp_b16.h): six products of total order <= 2 per K-block,
      // smallest first, fp32 accumulation.  Every activation tile is split pair by pair into the two K-blocks it is of the
      // next contraction.  One image per matrix serves its forward (ds_read_b128) and its transposed (ds_read_b64_tr_b16) walk.
      using namespace mlpb16;
      const auto w1 = walk1.opaque();  // (the images never change: opaque copies keep the operand loads at their MFMAs)
      const auto w2 = walk2.opaque();
      const auto w3 = walk3.opaque();
#include "mlp3_b16_tiles.inc"
      f32x16 acc[HT];
      f32x2 s1[HT][8], s2[HT][8];
      Split8p spa[2 * HT], spb[2 * HT];  // the B operands, alternating: h1 | h2 | d3 | d2 | d1
      // ---- layer 1: a1^T tiles, K = input columns
      bias_tiles(acc, b1s);
      contract_pipe<HT, 2 * DT, false, false>(
          acc, w1, [&](auto kb) __attribute__((always_inline)) -> const Split8p& { return spx[decltype(kb)::value]; }, NoFill{});
      static_for<HT>([&](auto tc) __attribute__((always_inline)) { silu_tile(tc, acc[decltype(tc)::value], s1[decltype(tc)::value], spa); });
      EBM_BLOCK_CUT();
      // ---- layer 2: a2^T tiles, K = units of layer 1
      bias_tiles(acc, b2s);
      contract_pipe<HT, 2 * HT, false, false>(
          acc, w2, [&](auto kb) __attribute__((always_inline)) -> const Split8p& { return spa[decltype(kb)::value]; }, NoFill{});
      static_for<HT>([&](auto tc) __attribute__((always_inline)) { silu_tile(tc, acc[decltype(tc)::value], s2[decltype(tc)::value], spb); });
      EBM_BLOCK_CUT();
      // ---- layer 3: a3^T tiles, K = units of layer 2; E += w4 silu(a3), d3 = w4 silu'(a3)
      bias_tiles(acc, b3s);
      contract_pipe<HT, 2 * HT, false, false>(
          acc, w3, [&](auto kb) __attribute__((always_inline)) -> const Split8p& { return spb[decltype(kb)::value]; }, NoFill{});
#include "mlp3_b16_energy.inc"
      EBM_BLOCK_CUT();
      if (!forward_only) {
        // ---- backward through W3: K = units of layer 3; d2 = (W3^T d3) s2
        zero_tiles(acc);
        contract_pipe<HT, 2 * HT, false, true>(
            acc, w3, [&](auto kb) __attribute__((always_inline)) -> const Split8p& { return spa[decltype(kb)::value]; }, NoFill{});
        static_for<HT>([&](auto tc) __attribute__((always_inline)) { back_tile(tc, acc[decltype(tc)::value], s2[decltype(tc)::value], spb); });
        EBM_BLOCK_CUT();
        // ---- backward through W2: K = units of layer 2; d1 = (W2^T d2) s1
        zero_tiles(acc);
        contract_pipe<HT, 2 * HT, false, true>(
            acc, w2, [&](auto kb) __attribute__((always_inline)) -> const Split8p& { return spb[decltype(kb)::value]; }, NoFill{});
        static_for<HT>([&](auto tc) __attribute__((always_inline)) { back_tile(tc, acc[decltype(tc)::value], s1[decltype(tc)::value], spa); });
        EBM_BLOCK_CUT();
        // ---- backward through W1: g^T tiles, K = units of layer 1 (image columns past dim are zero: the padding rows stay 0)
        contract_pipe<DT, 2 * HT, false, true>(
            g, w1, [&](auto kb) __attribute__((always_inline)) -> const Split8p& { return spa[decltype(kb)::value]; }, NoFill{});
      }
    } else {
      // ------------------------------------------------------------------------------------------------------------------
      // H = 128: v_mfma_f32_32x32x2_f32 on fp32 words in LDS at the conflict-free strides (mlp_wide_body.h contract<>: one LDS
      // word per A operand, requested one K-step ahead).  Exact fp32 products; 2 HT (3 HT + DT) 16 = 1 664 MFMAs of 64 cycles.
      int ms = m;  // (the lane parts of the addresses are opaque per step as well: the weight words are invariant over the loop)
      asm volatile("" : "+v"(ms));
      const auto fwd1 = [&](int t, int tk, int r) { return (32 * t + ms) * S1 + 32 * tk + row_of(r, hq); };
      const auto fwd2 = [&](int t, int tk, int r) { return (32 * t + ms) * S2 + 32 * tk + row_of(r, hq); };
      const auto bwd1 = [&](int t, int tk, int r) { return (32 * tk + row_of(r, hq)) * S1 + 32 * t + ms; };
      const auto bwd2 = [&](int t, int tk, int r) { return (32 * tk + row_of(r, hq)) * S2 + 32 * t + ms; };
      const auto bias_tiles = [&](f32x16 (&acc)[HT], const float* bsrc) __attribute__((always_inline)) {
#pragma unroll
        for (int t = 0; t < HT; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[t][r] = bsrc[32 * t + row_of(r, hq)];
      };
      const auto zero_tiles = [&](f32x16 (&acc)[HT]) __attribute__((always_inline)) {
#pragma unroll
        for (int t = 0; t < HT; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
      };
      // h = silu(a) in place, silu'(a) kept
      const auto silu_tiles = [&](f32x16 (&acc)[HT], f32x16 (&sd)[HT]) __attribute__((always_inline)) {
#pragma unroll
        for (int t = 0; t < HT; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float av = acc[t][r];
            const float sg = sigmoid_fast(av);
            const float hv = av * sg;
            acc[t][r] = hv;
            sd[t][r] = __builtin_fmaf(hv, 1.0f - sg, sg);  // silu'(a) = s + silu(a) (1 - s)
          }
      };
      f32x16 u[HT], v[HT], s1[HT], s2[HT];
      // ---- layer 1
      bias_tiles(u, b1s);
      contract<HT, DT>(u, W1s, fwd1, [&](int tk, int r) { return xr[tk][r]; });
      silu_tiles(u, s1);
      // ---- layer 2
      bias_tiles(v, b2s);
      contract<HT, HT>(v, W2s, fwd2, [&](int tk, int r) { return u[tk][r]; });
      silu_tiles(v, s2);
      // ---- layer 3: E += w4 silu(a3), d3 = w4 silu'(a3)
      bias_tiles(u, b3s);
      contract<HT, HT>(u, W3s, fwd2, [&](int tk, int r) { return v[tk][r]; });
      float e_part = 0.0f;
#pragma unroll
      for (int t = 0; t < HT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float av = u[t][r];
          const float sg = sigmoid_fast(av);
          const float w4 = w4s[32 * t + row_of(r, hq)];
          const float hv = av * sg;
          e_part = __builtin_fmaf(w4, hv, e_part);
          u[t][r] = w4 * __builtin_fmaf(hv, 1.0f - sg, sg);
        }
      energy = e_part + __shfl_xor(e_part, 32) + b4;  // the two K-halves hold the two halves of the rows
      if (!forward_only) {
        // ---- backward through W3, W2, W1
        zero_tiles(v);
        contract<HT, HT>(v, W3s, bwd2, [&](int tk, int r) { return u[tk][r]; });
#pragma unroll
        for (int t = 0; t < HT; ++t) v[t] *= s2[t];  // d2
        zero_tiles(u);
        contract<HT, HT>(u, W2s, bwd2, [&](int tk, int r) { return v[tk][r]; });
#pragma unroll
        for (int t = 0; t < HT; ++t) u[t] *= s1[t];  // d1
        contract<DT, HT>(g, W1s, bwd1, [&](int tk, int r) { return u[tk][r]; });
      }
    }
