// The layer-3 epilogue of the three-hidden-layer MLP's split-bf16 evaluation, shared as text like mlp3_b16_tiles.inc:
// E = w4 . silu(a3) + b4 and d3 = w4 * silu'(a3) as the K-blocks spa.  In scope: acc[HT] (a3), w4s, b4, hb, split_pair, spa;
// assigns `energy`.
      f32x2 e_pair = {0.0f, 0.0f};
      static_for<HT>([&](auto tc) __attribute__((always_inline)) {
        constexpr int t = decltype(tc)::value;
        static_for<8>([&](auto ic) __attribute__((always_inline)) {
          constexpr int i = decltype(ic)::value;
          // rows 32 t + 8 (i / 2) + 4 h + {2 (i % 2), + 1}
          const f32x2 w4p = *reinterpret_cast<const f32x2*>(w4s + 32 * t + 8 * (i >> 1) + 2 * (i & 1) + hb);
          const f32x2 av = pair_of<2 * i>(acc[t]);
          const f32x2 sg = {sigmoid_fast(av.x), sigmoid_fast(av.y)};
          const f32x2 hv = pmul<false>(av, sg);
          e_pair = pfma<false>(w4p, hv, e_pair);
          const f32x2 dd = pmul<false>(w4p, pfma<false>(hv, prsub<false>(1.0f, sg), sg));
          split_pair(spa[2 * t + (i >> 2)], std::integral_constant<int, (i & 3)>{}, dd);
        });
      });
      const float e_part = e_pair.x + e_pair.y;
      energy = e_part + __shfl_xor(e_part, 32) + b4;  // the two K-halves hold the two halves of the rows
