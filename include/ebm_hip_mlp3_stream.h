/*
 * ebm_hip_mlp3_stream.h -- companion of ebm_hip_mlp3.h: the three-hidden-layer SiLU MLP energy at hidden width 128 on the bf16
 * matrix pipe, 1 <= dim <= 128.  Exported by the same libebm_hip.so under the same ABI version (EBM_ABI_VERSION 9; ebm_hip.h and
 * ebm_hip_mlp3.h are unchanged, and their entries keep their shape tables: ebm_energy_grad_mlp3_f32 still refuses H = 128 at
 * dim 33).  Every convention is ebm_hip.h's: return codes, ebm_energy_t, the Philox coordinates, the stream argument.
 *
 * Two split 128 x 128 images do not fit a CU's LDS, so these entries keep W2 resident and stream W3 and W1 through two LDS
 * buffers from a PRE-SPLIT image in global memory, which the caller owns and hands over in ebm_energy_t.aux:
 *     kind = EBM_ENERGY_MLP3   n_comp = 128   dev0 = the packed parameters (ebm_hip_mlp3.h)   aux = the image
 * The image belongs to one parameter set: rebuild it (ebm_mlp3_image_f32) whenever the parameters change.
 */
#ifndef EBM_HIP_MLP3_STREAM_H
#define EBM_HIP_MLP3_STREAM_H

#include "ebm_hip_mlp3.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Size of the image in bytes: (n1 + 4) * 24 576 with n1 = 1, 2 or 4 W1 pieces for dim <= 32, <= 64 or <= 128, at hidden == 128
 * and 1 <= dim <= 128; 0 for every other shape.  Host arithmetic only: no device is touched.
 */
EBM_API size_t ebm_mlp3_image_bytes(int32_t hidden, int32_t dim);

/*
 * Build the image of the packed parameters `params` (device, the dev0 layout of ebm_hip_mlp3.h) into `image` (device,
 * ebm_mlp3_image_bytes(hidden, dim) bytes, 16-byte aligned) on `stream`: one small launch.  EBM_EDIM for a shape without an
 * image, EBM_EINVAL for a NULL or misaligned pointer.
 */
EBM_API int ebm_mlp3_image_f32(const float* params, int32_t hidden, int32_t dim, void* image, void* stream);

/*
 * ebm_energy_grad_mlp3_f32 and ebm_langevin_chain_mlp3_f32 (ebm_hip_mlp3.h) with the same argument lists and the same
 * contracts -- either output optional and the forward pass alone without grad_out; out of place with x_src == x allowed; the
 * reference's update order; native noise equal to the injected field bit for bit; a call cut in two equal to the whole;
 * k_steps == 0 copies the state -- computed by the streamed kernel.  Results agree with the exact-f32 kernel of the other
 * header to fp32 accuracy, not bit for bit (another instruction, another summation order).
 * Refusals, in this order and before any device access: a NULL energy (EBM_EINVAL); a kind other than EBM_ENERGY_MLP3
 * (EBM_EKIND); n_comp other than 128, dim outside 1 .. 128 (EBM_EDIM); NULL dev0, aux or state, a misaligned pointer (aux
 * included), n_chains < 0 or k_steps < 0 (EBM_EINVAL).
 */
EBM_API int ebm_energy_grad_mlp3_stream_f32(const ebm_energy_t* energy, const float* x, int64_t n_chains, int32_t dim,
                                            float* energy_out, float* grad_out, void* stream);
EBM_API int ebm_langevin_chain_mlp3_stream_f32(const ebm_energy_t* energy, const float* x_src, float* x, int64_t n_chains,
                                               int32_t dim, int32_t k_steps, float eta, float sqrt_eta, float noise_coef,
                                               const float* noise, uint64_t seed, uint64_t offset, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EBM_HIP_MLP3_STREAM_H */
