// The tile helpers of the three-hidden-layer MLP's split-bf16 evaluation and the state as K-blocks, shared as text by
// mlp3_eval.inc (H = 64, every image resident) and mlp3_stream_body.h (H = 128, W3 and W1 streamed).  In scope: mlpb16's names,
// HT, DT, hq (the lane's K-half, opaque per step) and the state xr[DT][16].  Defines hb, bias_tiles, zero_tiles, split_pair,
// silu_tile, back_tile and spx[2 DT].
      int hb = 4 * hq;
      asm volatile("" : "+v"(hb));
      // (pair arithmetic is spelled element by element throughout: no packed fp32 instruction in these units)
      const auto bias_tiles = [&](f32x16 (&acc)[HT], const float* bsrc) __attribute__((always_inline)) {
#pragma unroll
        for (int t = 0; t < HT; ++t)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float4 bq = *reinterpret_cast<const float4*>(bsrc + 32 * t + 8 * q + hb);
            acc[t][4 * q] = bq.x; acc[t][4 * q + 1] = bq.y; acc[t][4 * q + 2] = bq.z; acc[t][4 * q + 3] = bq.w;
          }
      };
      const auto zero_tiles = [&](f32x16 (&acc)[HT]) __attribute__((always_inline)) {
#pragma unroll
        for (int t = 0; t < HT; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
      };
      // pair p of a K-block: hi + mid + lo
      const auto split_pair = [&](Split8p& s, auto pc, f32x2 v) __attribute__((always_inline)) {
        constexpr int p = decltype(pc)::value;
        f32x2 r;
        pair_split_a<p, false>(s, r, v);
        pair_split_b<p, false>(s, r);
        pair_split_c<p>(s, r);
      };
      // pair i of tile t (registers 2 i, 2 i + 1) is pair i & 3 of K-block 2 t + (i >> 2) of the next contraction
      // a hidden layer's tile: h = silu(a) as two K-blocks, silu'(a) kept
      const auto silu_tile = [&](auto tc, const f32x16& acc, f32x2 (&sd)[8], Split8p (&sp)[2 * HT]) __attribute__((always_inline)) {
        constexpr int t = decltype(tc)::value;
        static_for<8>([&](auto ic) __attribute__((always_inline)) {
          constexpr int i = decltype(ic)::value;
          const f32x2 av = pair_of<2 * i>(acc);
          const f32x2 sg = {sigmoid_fast(av.x), sigmoid_fast(av.y)};
          const f32x2 hv = pmul<false>(av, sg);
          sd[i] = pfma<false>(hv, prsub<false>(1.0f, sg), sg);  // silu'(a) = s + silu(a) (1 - s)
          split_pair(sp[2 * t + (i >> 2)], std::integral_constant<int, (i & 3)>{}, hv);
        });
      };
      // a backward tile: d = T * silu' as two K-blocks
      const auto back_tile = [&](auto tc, const f32x16& acc, const f32x2 (&sd)[8], Split8p (&sp)[2 * HT]) __attribute__((always_inline)) {
        constexpr int t = decltype(tc)::value;
        static_for<8>([&](auto ic) __attribute__((always_inline)) {
          constexpr int i = decltype(ic)::value;
          split_pair(sp[2 * t + (i >> 2)], std::integral_constant<int, (i & 3)>{}, pmul<false>(pair_of<2 * i>(acc), sd[i]));
        });
      };
      // ---- the state as K-blocks
      Split8p spx[2 * DT];
      static_for<2 * DT>([&](auto kbc) __attribute__((always_inline)) {
        constexpr int kb = decltype(kbc)::value;
        static_for<4>([&](auto pc) __attribute__((always_inline)) {
          constexpr int p = decltype(pc)::value;
          split_pair(spx[kb], pc, (f32x2){xr[kb >> 1][8 * (kb & 1) + 2 * p], xr[kb >> 1][8 * (kb & 1) + 2 * p + 1]});
        });
      });
