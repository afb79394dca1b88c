// The set-up of a kernel on the three-hidden-layer MLP energy, shared as text by mlp3_body.h's chain / evaluation kernel and
// mlp3_hmc_body.h's transition kernel: the packed parameters, the LDS carve-up, the staging (once per launch) and the lane geometry.
// In scope: a.params, a.dim, a.n_chains and the constants HT, B16, H, DP, C1, S1, S2.  Defines dim, b4, b1s .. w4s, the fp32 words
// W1s / W2s / W3s or the images behind walk1 / walk2 / walk3, lane, m, h, sample, active and quads.
  const int dim = a.dim;
  const float* W1g = a.params;
  const float* b1g = W1g + H * dim;
  const float* W2g = b1g + H;
  const float* b2g = W2g + H * H;
  const float* W3g = b2g + H;
  const float* b3g = W3g + H * H;
  const float* w4g = b3g + H;
  const float b4 = w4g[H];
  // ---- the LDS carve-up and the staging (once per launch)
  float* const vecs = B16 ? wide_smem : wide_smem + 2 * H * S2 + H * S1;
  float* const b1s = vecs;
  float* const b2s = vecs + H;
  float* const b3s = vecs + 2 * H;
  float* const w4s = vecs + 3 * H;
  [[maybe_unused]] float* const W2s = wide_smem;        // fp32 words
  [[maybe_unused]] float* const W3s = W2s + H * S2;
  [[maybe_unused]] float* const W1s = W3s + H * S2;     // columns >= dim zero
  const mlpb16::lds_bytes img2 = (mlpb16::lds_bytes)(wide_smem + 4 * H);
  const mlpb16::lds_bytes img3 = img2 + mlpb16::image_bytes(H, H);
  const mlpb16::lds_bytes img1 = img3 + mlpb16::image_bytes(H, H);
  if constexpr (B16) {
    mlpb16::stage_image<H, H>(W2g, H, H, img2, kBlock);
    mlpb16::stage_image<H, H>(W3g, H, H, img3, kBlock);
    mlpb16::stage_image<H, C1>(W1g, H, dim, img1, kBlock);  // columns >= dim zero: the padding rows of dE/dx come out 0
  } else {
    for (int i = threadIdx.x; i < H * H; i += kBlock) {
      W2s[(i / H) * S2 + (i % H)] = W2g[i];
      W3s[(i / H) * S2 + (i % H)] = W3g[i];
    }
    for (int i = threadIdx.x; i < H * DP; i += kBlock) {
      const int row = i / DP, c = i - row * DP;
      W1s[row * S1 + c] = c < dim ? W1g[row * dim + c] : 0.0f;
    }
  }
  for (int i = threadIdx.x; i < H; i += kBlock) {
    b1s[i] = b1g[i];
    b2s[i] = b2g[i];
    b3s[i] = b3g[i];
    w4s[i] = w4g[i];
  }
  __syncthreads();

  const int lane = threadIdx.x & 63;
  [[maybe_unused]] const mlpb16::Walk<H, C1> walk1(img1, B16 ? lane : 0);
  [[maybe_unused]] const mlpb16::Walk<H, H> walk2(img2, B16 ? lane : 0);
  [[maybe_unused]] const mlpb16::Walk<H, H> walk3(img3, B16 ? lane : 0);
  const int m = lane & 31, h = lane >> 5;
  const int64_t sample = ((int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * 32 + m;
  const bool active = sample < a.n_chains;  // chains past n are neither loaded nor stored
  const bool quads = (dim & 3) == 0;
