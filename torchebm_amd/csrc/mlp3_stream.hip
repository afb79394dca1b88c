// The three-hidden-layer SiLU MLP energy at hidden width 128 on the bf16 matrix pipe with W3 and W1 streamed from a pre-split
// image (mlp3_stream_body.h; docs/design/mlp3_stream.md): the four entries of include/ebm_hip_mlp3_stream.h, their refusals,
// the image kernel and the three instantiations (DT = 1 / 2 / 4: dim <= 32 / 64 / 128).
#include "../../include/ebm_hip_mlp3_stream.h"
#include "mlp3_stream_body.h"

namespace ebm {
namespace mlp3 {
namespace {

constexpr int kStreamHidden = 128, kStreamMaxDim = 128;

int stream_cols(int32_t dim) { return dim <= 32 ? 32 : (dim <= 64 ? 64 : 128); }  // C1: the width of a W1 piece

// The image: [W1 pieces 0 .. n1 - 1][W3 slabs 0 .. 3], 24 576 bytes each.  W1 piece p = the three splits [R1][C1] of rows
// R1 p .. R1 p + R1 - 1 (R1 = 4096 / C1) exactly as stage_image<R1, C1> would write them, columns past dim zero; W3 slab s = the
// three splits [32][128] of rows 32 s .. 32 s + 31 (mlp_b16.h's slab format).  One thread per (row, four columns).
__global__ __launch_bounds__(256) void mlp3_build_image(const float* __restrict__ params, int dim, int c1, char* __restrict__ out) {
  using namespace mlpb16;
  constexpr int H = kStreamHidden;
  constexpr uint32_t SPLIT = kSlabBytes / 3u;  // R1 * 2 C1 = 32 * 2 * 128
  const int q1 = c1 / 4, n_w1 = H * q1, n1 = stream_pieces(c1), r1 = 4096 / c1;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_w1 + H * (H / 4)) return;
  const float* w;
  int row, cq, cols;
  char* dst;
  if (i < n_w1) {
    row = i / q1; cq = i - row * q1; w = params; cols = dim;
    const uint32_t rl = (uint32_t)(row % r1);
    dst = out + (size_t)(row / r1) * kSlabBytes
          + (c1 == 32 ? Img<32>::atom(rl, (uint32_t)cq) : (c1 == 64 ? Img<64>::atom(rl, (uint32_t)cq) : Img<128>::atom(rl, (uint32_t)cq)));
  } else {
    const int j = i - n_w1;
    row = j / (H / 4); cq = j - row * (H / 4); w = params + H * dim + H + H * H + H; cols = H;
    dst = out + (size_t)(n1 + row / kSlabRows) * kSlabBytes + Img<kSlabCols>::atom((uint32_t)(row % kSlabRows), (uint32_t)cq);
  }
  bf16x4 hi, mid, lo;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int c = 4 * cq + e;
    const float v = c < cols ? w[(size_t)row * cols + c] : 0.0f;
    __bf16 s0, s1, s2;
    gauss3::split3(v, s0, s1, s2);
    hi[e] = s0; mid[e] = s1; lo[e] = s2;
  }
  *reinterpret_cast<bf16x4*>(dst) = hi;
  *reinterpret_cast<bf16x4*>(dst + SPLIT) = mid;
  *reinterpret_cast<bf16x4*>(dst + 2u * SPLIT) = lo;
}

// kind, then the shape, then the pointers: all before any device access
int check_stream(const char* who, const ebm_energy_t* energy, int32_t dim) {
  if (!energy) return fail(EBM_EINVAL, "%s: energy descriptor is NULL", who);
  if (energy->kind != EBM_ENERGY_MLP3) return fail(EBM_EKIND, "%s: this entry takes EBM_ENERGY_MLP3 only (got kind %d)", who, energy->kind);
  if (energy->n_comp != kStreamHidden) return fail(EBM_EDIM, "%s: hidden width %d (the streamed kernel takes 128)", who, energy->n_comp);
  if (dim < 1 || dim > kStreamMaxDim) return fail(EBM_EDIM, "%s: dim %d outside 1 .. %d", who, dim, kStreamMaxDim);
  if (!energy->dev0) return fail(EBM_EINVAL, "%s: the energy needs the packed parameter pointer", who);
  if (!energy->aux) return fail(EBM_EINVAL, "%s: the energy needs the pre-split image (ebm_mlp3_image_f32) in aux", who);
  if (!aligned16(energy->aux)) return fail(EBM_EINVAL, "%s: the image must be 16-byte aligned", who);
  return 0;
}

int dispatch_stream(const Args& a, const ebm_energy_t* energy, hipStream_t st, const char* who) {
  const char* image = reinterpret_cast<const char*>(energy->aux);
  if (a.dim <= 32) return launch_stream<1>(a, image, st, who);
  if (a.dim <= 64) return launch_stream<2>(a, image, st, who);
  return launch_stream<4>(a, image, st, who);
}

}  // namespace
}  // namespace mlp3
}  // namespace ebm

using namespace ebm;

extern "C" {

size_t ebm_mlp3_image_bytes(int32_t hidden, int32_t dim) {
  if (hidden != mlp3::kStreamHidden || dim < 1 || dim > mlp3::kStreamMaxDim) return 0;
  return (size_t)(mlp3::stream_pieces(mlp3::stream_cols(dim)) + 4) * mlpb16::kSlabBytes;
}

int ebm_mlp3_image_f32(const float* params, int32_t hidden, int32_t dim, void* image, void* stream) {
  const char* who = "ebm_mlp3_image_f32";
  if (ebm_mlp3_image_bytes(hidden, dim) == 0)
    return fail(EBM_EDIM, "%s: no image for hidden width %d at dim %d (128 at 1 .. 128 only)", who, hidden, dim);
  if (!params || !image) return fail(EBM_EINVAL, "%s: NULL pointer", who);
  if (!aligned16(image)) return fail(EBM_EINVAL, "%s: the image must be 16-byte aligned", who);
  const int c1 = mlp3::stream_cols(dim), work = hidden * (c1 / 4) + hidden * (hidden / 4);
  hipLaunchKernelGGL(mlp3::mlp3_build_image, dim3((work + 255) / 256), dim3(256), 0, (hipStream_t)stream, params, dim, c1,
                     static_cast<char*>(image));
  return check_launch(who);
}

int ebm_energy_grad_mlp3_stream_f32(const ebm_energy_t* energy, const float* x, int64_t n_chains, int32_t dim, float* energy_out,
                                    float* grad_out, void* stream) {
  const char* who = "ebm_energy_grad_mlp3_stream_f32";
  if (int r = mlp3::check_stream(who, energy, dim)) return r;
  if (!x) return fail(EBM_EINVAL, "%s: state pointer is NULL", who);
  if (n_chains < 0) return fail(EBM_EINVAL, "%s: n_chains < 0", who);
  if (!aligned16(x) || (grad_out && !aligned16(grad_out))) return fail(EBM_EINVAL, "%s: x / grad_out must be 16-byte aligned", who);
  if (n_chains == 0 || (!energy_out && !grad_out)) return 0;
  mlp3::Args a{};
  a.x_src = x; a.n_chains = n_chains; a.dim = dim; a.k_steps = 0;
  a.params = static_cast<const float*>(energy->dev0);
  a.energy_out = energy_out; a.grad_out = grad_out;
  return mlp3::dispatch_stream(a, energy, (hipStream_t)stream, who);
}

int ebm_langevin_chain_mlp3_stream_f32(const ebm_energy_t* energy, const float* x_src, float* x, int64_t n_chains, int32_t dim,
                                       int32_t k_steps, float eta, float sqrt_eta, float noise_coef, const float* noise,
                                       uint64_t seed, uint64_t offset, void* stream) {
  const char* who = "ebm_langevin_chain_mlp3_stream_f32";
  if (int r = mlp3::check_stream(who, energy, dim)) return r;
  if (!x_src || !x) return fail(EBM_EINVAL, "%s: state pointer is NULL", who);
  if (n_chains < 0 || k_steps < 0) return fail(EBM_EINVAL, "%s: n_chains=%lld k_steps=%d", who, (long long)n_chains, k_steps);
  if (!aligned16(x_src) || !aligned16(x) || (noise && !aligned16(noise)))
    return fail(EBM_EINVAL, "%s: x_src / x / noise must be 16-byte aligned", who);
  const size_t state_bytes = (size_t)n_chains * (size_t)dim * sizeof(float);
  if (x_src != x) {
    const uintptr_t s0 = (uintptr_t)x_src, x0 = (uintptr_t)x;
    if (s0 < x0 + state_bytes && x0 < s0 + state_bytes)
      return fail(EBM_EINVAL, "%s: x_src overlaps x without being x", who);
  }
  const hipStream_t st = (hipStream_t)stream;
  if (n_chains == 0) return 0;
  if (k_steps == 0) {  // no step: the output is the start state
    if (x_src == x) return 0;
    const hipError_t e = hipMemcpyAsync(x, x_src, state_bytes, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) return 0;
    set_error("%s: copying x_src into x failed: %s", who, hipGetErrorString(e));
    return (int)e;
  }
  mlp3::Args a{};
  a.x_src = x_src; a.x = x; a.n_chains = n_chains; a.dim = dim; a.k_steps = k_steps;
  a.eta = eta; a.sqrt_eta = sqrt_eta; a.noise_coef = noise_coef;
  a.noise = noise;
  a.key = RngKey{(uint32_t)seed, (uint32_t)(seed >> 32)};
  a.step0 = offset;
  a.params = static_cast<const float*>(energy->dev0);
  return mlp3::dispatch_stream(a, energy, st, who);
}

}  // extern "C"
