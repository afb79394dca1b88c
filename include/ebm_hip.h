/*
 * ebm_hip.h -- C ABI of libebm_hip.so: the MI355X (gfx950) kernels behind torchebm's
 * Langevin / HMC sampler inner loop.
 *
 * The reference (soran-ghaderi/torchebm) is a pure-Python library with no FFI layer;
 * its boundary for this path is the Python class API.  These entry
 * points are what a ctypes binding inside the reference would call; each one names the
 * reference code it replaces (paths relative to the reference checkout).
 *
 * Conventions (all entry points)
 *   - the caller owns every buffer; the library never allocates or frees device memory
 *     and keeps no pointer after a call returns;
 *   - device pointers are fp32, row-major contiguous, 16-byte aligned;
 *   - `stream` is a hipStream_t (NULL = the default stream); calls only ENQUEUE work
 *     and return, they never synchronise the device or the host;
 *   - return value: 0 = ok, >0 = a hipError_t from the launch, <0 = EBM_E* argument
 *     error; the text is available from ebm_last_error_string() (thread local);
 *   - no C++ exception crosses the boundary; no mutable global state; the library reads no
 *     environment variable (the kernel-selection switches of scripts/ -- EBM_GAUSS_ROWS and
 *     friends -- exist only in builds made with -DEBM_AB_SWITCHES; tests/test_abi.py checks
 *     that the shipped object does not import getenv).
 *
 * Random numbers ("native RNG", used when a noise pointer is NULL)
 *   Philox4x32-10 keyed by `seed`.  For step s (64-bit, = offset + local step index)
 *   and flat element e:  counter = { lo32(e/4), hi32(e/4), lo32(s), hi32(s) }, the
 *   four 32-bit outputs o0..o3 give, by Box-Muller on (o0,o1) and (o2,o3), the four
 *   standard normals of elements 4*(e/4)+0..3.  Uniforms (HMC accept) use
 *   u = (o[e%4] >> 8) * 2^-24 in [0,1).  The stream therefore depends only on
 *   (seed, offset, step, element) -- never on launch geometry -- and the fused k-step
 *   kernels, the per-step kernel and ebm_noise_fill_f32 all draw the same field.
 */
#ifndef EBM_HIP_H
#define EBM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EBM_ABI_VERSION 9

#if defined(__GNUC__)
#define EBM_API __attribute__((visibility("default")))
#else
#define EBM_API
#endif

/* argument errors (negative); positive return values are hipError_t */
#define EBM_EINVAL  (-1)  /* bad size / NULL pointer / misaligned pointer          */
#define EBM_EKIND   (-2)  /* unknown or unsupported energy kind for this entry     */
#define EBM_EDIM    (-3)  /* dim outside the range the fused kernel supports       */

/* Analytic energies the kernels fuse (reference: torchebm/core/base_model.py). */
enum {
  EBM_ENERGY_DOUBLE_WELL = 0, /* E = h * sum_j (x_j^2 - b^2)^2   base_model.py:130-148  s[0]=h  s[1]=(float)(b*b)           */
  EBM_ENERGY_HARMONIC    = 1, /* E = (0.5*k) * sum_j x_j^2       base_model.py:213-229  s[0]=(float)(0.5*k)                 */
  EBM_ENERGY_GAUSSIAN    = 2, /* E = 0.5 d^T P d, d = x - mu     base_model.py:151-210  dev0=mu[dim] dev1=P[dim*dim] (P=cov^-1)
                                 aux = NULL, or (since ABI version 4) the device image that ebm_gauss_prec_image_f32 built from
                                 THIS dev1 -- multiples of 4 from 132 to 512, and (ABI version 5) the widths 158 .. 254 that
                                 are NOT a multiple of 4, where the image holds one shifted copy per alignment class (4 for an
                                 odd width, 2 for width = 2 mod 4; ebm_gauss_prec_image_bytes gives the size, 0 = no image at
                                 this width): the tiled kernels then move their slabs of P by LDS-direct loads instead of
                                 loading, splitting and storing fp32 rows every stage, and the streamed kernels of the shifted
                                 widths (Langevin 158 .. 254, HMC 161 .. 254) REQUIRE it (without it those widths take the
                                 lane-group kernels).  A stale image gives the old matrix's samples; NULL is always safe.     */
  EBM_ENERGY_GMM         = 3, /* E = -logsumexp_k(logw_k - |x-mu_k|^2 * s[0])  (not in the reference: SURVEY §8 a6)
                                 s[0]=1/(2 sigma^2)  s[1]=1/sigma^2  n_comp=K  dev0=mu[K*dim] dev1=logw[K]
                                 aux = NULL, or device int32[1]: bit v set <=> the component means differ somewhere in
                                 columns 4v..4v+3 (v < 8).  A hint, read by the kernel itself: columns all components
                                 share drop out of the responsibilities, and when the mask is 1 (a mixture of a plane
                                 embedded in the first coordinates, e.g. BASELINE config 3's ring) the one-lane-per-chain
                                 kernels (dim 16 / 32, K <= 8) run their K x dim passes over four columns only.
                                 A wrong mask gives wrong samples; NULL is always safe.                                    */
  EBM_ENERGY_MLP         = 4, /* E = w3 . silu(W2 silu(W1 x + b1) + b2) + b3   (the energy of the reference's
                                 examples/20-training/01-mcmc-losses/02-persistent-cd/main.py:21-31)
                                 n_comp = hidden width H (64 or 128; 256 only in a build made with `make H256=1`), dim <= 128 (the reference's benchmark network
                                 benchmarks/registry.py:372-387 at dim 8 / 32 / 128),
                                 dev0 = packed fp32 parameters W1[H,dim] b1[H] W2[H,H] b2[H] w3[H] b3[1] (torch Linear layout).
                                 Supported by ebm_langevin_chain_f32, ebm_energy_grad_f32 and ebm_hmc_chain_f32 (EBM_EDIM for
                                 other widths).  (H = 256, where built, reads
                                 the weights from dev0 throughout the launch: dev0 must then be 16-byte aligned.)
                                 aux = NULL, or (H = 128, 64 < dim <= 128, since ABI version 4) the device image that
                                 ebm_mlp_w1_image_f32 built from THIS dev0 (cast to const int32_t*): with it the Langevin
                                 and energy / gradient entries run their contractions on the bf16 matrix pipe with
                                 three-way split operands (fp32 accuracy) as the narrower shapes always do; without it on
                                 the exact-f32 matrix instruction (1.6x slower).  A stale image gives the old network's
                                 samples; NULL is always safe.                                                            */
  /* The three test landscapes of the reference's core (since ABI version 9): scalars only, dev0 = dev1 = aux = NULL, n_comp = 0.
     Lane-group kernels, dim <= 1024 (EBM_EDIM above); taken by ebm_langevin_chain_f32, ebm_langevin_heun_chain_f32,
     ebm_hmc_chain_f32, ebm_descent_chain_f32, ebm_energy_grad_f32 and ebm_diag_layout, not by ebm_hmc_chain_audit_f32.
     Tolerance tier: sums run in another order than torch's (docs/design/landscapes.md).                                   */
  EBM_ENERGY_ROSENBROCK  = 5, /* E = sum_{i<dim-1} (a - x_i)^2 + b (x_{i+1} - x_i^2)^2   base_model.py:232-264
                                 s[0]=a  s[1]=b;  dim >= 2 (EBM_EDIM below: the reference raises there)                   */
  EBM_ENERGY_ACKLEY      = 6, /* E = -a exp(-b sqrt(mean_j x_j^2)) - exp(mean_j cos(c x_j)) + a + e   base_model.py:267-294
                                 s[0]=a  s[1]=b  s[2]=c.  s[2] == (float)(2 pi) evaluates cos / sin(c x) as cospi / sinpi(2 x)
                                 (no argument product, no range reduction), any other c as cos / sin of the fp32 product.
                                 The gradient at x = 0 is NaN in every coordinate, as autograd's is (inf * 0).             */
  EBM_ENERGY_RASTRIGIN   = 7  /* E = a dim + sum_j x_j^2 - a cos(2 pi x_j)               base_model.py:297-316   s[0]=a   */
};

typedef struct ebm_energy {
  int32_t kind;        /* EBM_ENERGY_*                              */
  int32_t n_comp;      /* mixture components (GMM), else 0          */
  float   s[4];        /* scalar parameters, see the enum           */
  const float* dev0;   /* device parameter arrays, see the enum     */
  const float* dev1;
  const int32_t* aux;  /* optional device hints, see the enum (NULL: none) */
} ebm_energy_t;

/* noise kinds for ebm_noise_fill_f32 */
enum { EBM_NOISE_NORMAL = 0, EBM_NOISE_UNIFORM = 1, EBM_NOISE_RAW_U32 = 2 };

/* mass kinds for the HMC / leapfrog entries (reference: samplers/hmc.py:92-159, integrators/leapfrog.py:91-101) */
enum { EBM_MASS_NONE = 0, EBM_MASS_SCALAR = 1, EBM_MASS_DIAG = 2 };

EBM_API int ebm_version(void);
EBM_API const char* ebm_last_error_string(void);

/*
 * One Euler-Maruyama step with an externally supplied gradient.
 * Replaces BaseSDERungeKuttaIntegrator.step with the EulerMaruyama tableau
 * (core/base_integrator.py:673-731, integrators/euler_maruyama.py:55-65) and is the HIP
 * counterpart of the Triton POC kernel (cuda/fused_langevin.py:34-62).
 * Arithmetic, each op rounded to fp32, no FMA contraction:
 *     x1  = x - eta * grad            (= x + eta*(1.0*drift), drift = -grad)
 *     dw  = eps * sqrt_eta            (sqrt_eta  = (float) sqrt((double)eta))
 *     out = x1 + noise_coef * dw      (noise_coef = (float) sqrt(2*sigma^2), 0 => ODE step, no noise drawn)
 *     out = clamp(out, cmin, cmax)    if clamp_on   (samplers/langevin_dynamics.py:166-167)
 * eps = noise[e] if noise != NULL, else the native RNG field at step `offset`.
 * `out` may alias `x` (the same pointer: every element is read before it is written, by the lane that writes it; a shifted
 * overlap is not supported).  `grad` may be NULL (zero drift).  Exactly n_elem floats of `out` are written, whether n_elem is
 * a multiple of 4 (streaming float4 kernel) or not (float4 groups and a scalar tail): both forms give the same values.
 */
EBM_API int ebm_langevin_step_f32(const float* x, const float* grad, float* out, const float* noise,
                          int64_t n_elem, float eta, float sqrt_eta, float noise_coef,
                          int32_t clamp_on, float cmin, float cmax,
                          uint64_t seed, uint64_t offset, void* stream);

/*
 * The same step with a TENSOR diffusion coefficient D instead of the scalar noise scale
 * (BaseSDERungeKuttaIntegrator.step(..., diffusion=D), core/base_integrator.py:652-671, 724-729):
 *     out = (x - eta * grad) + sqrt(2 * D_e) * (eps * sqrt_eta),      D_e = diffusion[e % diffusion_period]
 * with (2.0 * D) ** 0.5 evaluated as torch does (fp32 product, correctly rounded fp32 square root).
 * diffusion_period = 1 (a 0-dim tensor), the row width (one value per coordinate) or n_elem (a full field); it must
 * divide n_elem.  No clamp (the integrator has none).  `out` may alias `x`, `grad` may be NULL.
 */
EBM_API int ebm_langevin_step_diffusion_f32(const float* x, const float* grad, float* out, const float* noise,
                                            const float* diffusion, int64_t diffusion_period, int64_t n_elem, float eta,
                                            float sqrt_eta, uint64_t seed, uint64_t offset, void* stream);

/*
 * The same step with the RNG coordinates read from DEVICE memory: rng_state = {seed, step} (two
 * uint64).  Kernel arguments are frozen when a launch is captured into a HIP graph; keeping
 * (seed, step) in a device buffer that the graph itself advances lets one captured
 * "gradient + update" iteration be replayed k times per sample() call with fresh noise every time
 * (the launch-bound autograd route of BASELINE config 5).  No injected-noise form.
 * The call equals ebm_langevin_step_f32 with seed = rng_state[0], offset = rng_state[1] (all 64 bits of both): this entry has
 * no step_delta argument, the stored step IS the step.  The entries that take one (ebm_hmc_accept_dev_f32,
 * ebm_noise_fill_dev_f32, the ABI 6 entries below) draw at rng_state[1] + step_delta, a 64-bit sum.  rng_state is only read.
 */
EBM_API int ebm_langevin_step_dev_f32(const float* x, const float* grad, float* out, int64_t n_elem,
                                      float eta, float sqrt_eta, float noise_coef,
                                      int32_t clamp_on, float cmin, float cmax,
                                      const uint64_t* rng_state, void* stream);

/*
 * k fused Langevin steps for an analytic energy: gradient + EM update + noise + clamp
 * + thinned trajectory stores, state resident in registers/LDS across the k steps.
 * Replaces the hot loop of LangevinDynamics.sample (samplers/langevin_dynamics.py:154-185)
 * including BaseModel.gradient (core/base_model.py:62-127) for the fused energies.
 *   x            [n_chains, dim]    in/out
 *   coef_table   NULL, or device float[k_steps][4] = {eta_i, sqrt_eta_i, noise_coef_i, 0}
 *                (pre-expanded schedulers, core/schedulable.py:55-75); when NULL the three
 *                scalars are used for every step
 *   traj         NULL, or [n_chains, k_steps/thin, dim]; row j is the state after step (j+1)*thin
 *   diag_partials NULL, or the per-block diagnostics records of the k_steps/thin kept steps (see
 *                ebm_diag_layout / ebm_diag_finish_f32 below): the sampler diagnostics of
 *                samplers/langevin_dynamics.py:170-185 (population mean / var, mean energy) without leaving
 *                the launch.  EBM_EDIM / EBM_EKIND when this energy / dim has no in-kernel form (ask
 *                ebm_diag_layout first).
 *   noise        NULL (native RNG, steps offset .. offset+k-1), or [k_steps, n_chains, dim]
 *   clamp_on     a flag word (ABI 8; 0 / 1 mean what they always did): EBM_CHAIN_CLAMP = 1 clamps to [cmin, cmax];
 *                EBM_CHAIN_CONTRACTED = 2 PERMITS contracted arithmetic -- x^2 - b^2 and x - eta g as fused multiply-adds, the
 *                coefficient noise_coef * sqrt_eta folded into the Box-Muller radius -- where a kernel has that form (element-wise
 *                energies, the plain call: constant coefficients, no clamp, no trajectory, no records, the kernels' own draws:
 *                8 of 76 vector instructions per float4 group-step fewer); every other call ignores the bit.  Not the
 *                reference's rounding (core/base_integrator.py:711-731 rounds every multiply and add): same law, same Philox
 *                field, last-bit differences per step.  Host side: `sampler.fused_arithmetic = True` on LangevinDynamics.
 */
#define EBM_CHAIN_CLAMP      1
#define EBM_CHAIN_CONTRACTED 2
EBM_API int ebm_langevin_chain_f32(const ebm_energy_t* energy, float* x, int64_t n_chains, int32_t dim,
                           int32_t k_steps, float eta, float sqrt_eta, float noise_coef,
                           const float* coef_table, int32_t clamp_on, float cmin, float cmax,
                           int32_t thin, float* traj, float* diag_partials, const float* noise,
                           uint64_t seed, uint64_t offset, void* stream);

/*
 * ebm_langevin_chain_f32 out of place: the chains start from `x_src` and their final state is stored to `x`; `x_src` is only
 * read.  Every other argument, every result (x, traj, diag_partials) and every error is that of ebm_langevin_chain_f32
 * called on a copy of x_src -- the same states bit for bit, for every energy -- without the copy where the kernel allows it:
 * the element-wise kernels (EBM_ENERGY_DOUBLE_WELL, EBM_ENERGY_HARMONIC on the flat layout) load x_src once and store x
 * once; for every other kernel family the entry copies x_src into x on `stream` first and continues in place.
 *   x_src        [n_chains, dim]    read-only, 16-byte aligned; NULL or x itself: the in-place call (identical to
 *                                   ebm_langevin_chain_f32)
 *   x            [n_chains, dim]    out (in/out when x_src is NULL or x)
 * The two ranges must be the same or disjoint: any other overlap returns EBM_EINVAL before anything is launched.  With
 * k_steps == 0, x receives x_src.  An injected `noise` is allowed with a distinct x_src.  A call cut into several launches
 * (records of a long run) passes x_src to the first launch only and continues in place on x.  Same ABI version: no
 * existing signature or struct changes.
 */
EBM_API int ebm_langevin_chain_from_f32(const ebm_energy_t* energy, const float* x_src, float* x, int64_t n_chains, int32_t dim,
                           int32_t k_steps, float eta, float sqrt_eta, float noise_coef,
                           const float* coef_table, int32_t clamp_on, float cmin, float cmax,
                           int32_t thin, float* traj, float* diag_partials, const float* noise,
                           uint64_t seed, uint64_t offset, void* stream);

/*
 * The same k fused steps with the reference's Heun (improved Euler) drift update,
 * LangevinDynamics(integrator="heun"): tableau a = ((), (1,)), b = (1/2, 1/2) (integrators/heun.py)
 * evaluated in the op order of BaseSDERungeKuttaIntegrator (core/base_integrator.py:387-397, 711-731):
 *   k0 = -grad E(x);  x1 = x + eta*(1*k0);  k1 = -grad E(x1);
 *   x' = x + eta*(0.5*k0 + 0.5*k1) + noise_coef*(eps*sqrt_eta)
 * Two gradient evaluations per step, one noise draw (same Philox coordinates as the EM chain).
 * Arguments as ebm_langevin_chain_f32; DoubleWell / Harmonic / Gaussian / mixture energies
 * (EBM_ENERGY_MLP returns EBM_EKIND).
 */
EBM_API int ebm_langevin_heun_chain_f32(const ebm_energy_t* energy, float* x, int64_t n_chains, int32_t dim,
                           int32_t k_steps, float eta, float sqrt_eta, float noise_coef,
                           const float* coef_table, int32_t clamp_on, float cmin, float cmax,
                           int32_t thin, float* traj, float* diag_partials, const float* noise,
                           uint64_t seed, uint64_t offset, void* stream);

/*
 * n_mh fused HMC transitions for an analytic energy (or EBM_ENERGY_MLP): momentum draw, Hamiltonian,
 * L leapfrog steps (safe mode: force clamp +-1e6, NaN scrub), Metropolis accept.
 * Replaces the hot loop of HamiltonianMonteCarlo.sample (samplers/hmc.py:243-312),
 * LeapfrogIntegrator.integrate (integrators/leapfrog.py:116-187) and the clamps of
 * core/base_integrator.py:875-889.
 *   x            [n_chains, dim]   in/out
 *   eps_table    NULL, or device float[n_mh] (scheduled step size per MH step)
 *   mass         EBM_MASS_*: none / scalar (a double, as the Python float it mirrors: the kernel uses
 *                (float)sqrt(m) for the momentum draw, (float)m for the kinetic energy and
 *                (float)max(m,1e-10) in the drift) / device float[dim]
 *   traj         NULL, or [n_chains, n_mh/thin, dim]
 *   diag_partials NULL, or the per-block diagnostics records of the n_mh/thin kept transitions (samplers/hmc.py:294-310:
 *                population mean / var, mean clamped energy, acceptance rate), see ebm_diag_layout below
 *   accept_mask  NULL, or uint8[n_mh, n_chains]   (1 = proposal accepted)
 *   accept_count NULL, or uint32[n_mh], must be zeroed by the caller; receives the number
 *                of accepted chains per MH step (wavefront ballot + one atomic per wave)
 *   p_noise      NULL (native RNG), or [n_mh, n_chains, dim] standard normals
 *   u            NULL (native RNG), or [n_mh, n_chains] uniforms in [0,1)
 * Native RNG consumes two steps per transition: offset+2t (momentum), offset+2t+1 (uniform).
 */
EBM_API int ebm_hmc_chain_f32(const ebm_energy_t* energy, float* x, int64_t n_chains, int32_t dim,
                      int32_t n_mh, int32_t n_leapfrog, float eps, const float* eps_table,
                      int32_t mass_kind, double mass_scalar, const float* mass_diag,
                      int32_t thin, float* traj, float* diag_partials, uint8_t* accept_mask, uint32_t* accept_count,
                      const float* p_noise, const float* u,
                      uint64_t seed, uint64_t offset, void* stream);

/*
 * Leapfrog sub-steps with an externally supplied force (opaque drift closure):
 * LeapfrogIntegrator.step / .integrate (integrators/leapfrog.py:63-187).
 *   kick_drift:  f = clamp(force) if safe;  p_half = p + (0.5*eps)*f;  x_new = x + eps*p_half [/ max(m,1e-10)]
 *   kick:        f = clamp(force) if safe;  p_new  = p_half + (0.5*eps)*f;  if safe: nan_to_num(x_new, p_new)
 * `x_new` of kick is updated in place (the NaN scrub: an element that needs none is not stored to and keeps its bits);
 * outputs may alias inputs element for element: x_new == x and p_half == p (kick_drift), p_new == p_half (kick).  `force`
 * and `mass_diag` are only read and may alias no output.  The diagonal mass is clamped per element, (m < 1e-10) ? 1e-10 : m,
 * so a NaN entry stays NaN; nan_to_num sends NaN to 0 and +-inf to +-FLT_MAX.
 */
EBM_API int ebm_leapfrog_kick_drift_f32(const float* x, const float* p, const float* force,
                                float* x_new, float* p_half, int64_t n_chains, int32_t dim,
                                float eps, int32_t mass_kind, double mass_scalar,
                                const float* mass_diag, int32_t safe, void* stream);
EBM_API int ebm_leapfrog_kick_f32(float* x_new, const float* p_half, const float* force, float* p_new,
                          int64_t n_elem, float eps, int32_t safe, void* stream);

/*
 * Metropolis accept for the per-step HMC path (samplers/hmc.py:277-292):
 *   d = clamp(h0 - h1, -50, 50); a = min(1, exp(d)); acc = u < a; x = acc ? x_prop : x
 * u = u_or_null[c], or the native uniform field at step `offset`, element c.
 * The clamp and the minimum propagate NaN: a NaN Hamiltonian (or inf - inf) rejects.  The comparison is strict: an injected
 * u = 1 rejects at a = 1, u = 0 accepts at the clamped a = e^-50.  Rejected rows of x are not stored to.
 *   accept_mask  NULL, or uint8[n_chains]: 1 = accepted, every entry written
 *   accept_count NULL, or uint32[1] that the call ADDS the number of accepted chains to (atomics; zero it first for a count
 *                of this call alone)
 */
EBM_API int ebm_hmc_accept_f32(float* x, const float* x_prop, const float* h0, const float* h1,
                       const float* u, uint8_t* accept_mask, uint32_t* accept_count,
                       int64_t n_chains, int32_t dim, uint64_t seed, uint64_t offset, void* stream);

/*
 * ABI 6 -- the AUDIT form of ebm_hmc_chain_f32 for the element-wise energies (double well, harmonic; dim <= 256; no records):
 * same arguments, same transitions, but the trajectory is the reference's safe-mode leapfrog step LITERALLY
 * (torchebm/integrators/leapfrog.py:156-185): the force re-evaluated at the top of every step, two separate half kicks, every
 * multiply and add rounded on its own, the drift divided by max(m, 1e-10) per step, both nan_to_num_ scrubs on every step,
 * energy and force re-evaluated at the top of every transition (samplers/hmc.py:243-256).  Given the same accept decisions the
 * state is the reference's BIT FOR BIT (tests/test_hmc_audit_gpu.py: torch.equal on the recorded fixtures).  For tests: it exists
 * so that what the fast body of ebm_hmc_chain_f32 trades away (merged kicks, fused multiply-adds, the hoisted eps / m) is a measured
 * quantity; it costs 2 L + 2 evaluations per transition where the fast body spends L.  EBM_EKIND for other energies.
 */
EBM_API int ebm_hmc_chain_audit_f32(const ebm_energy_t* energy, float* x, int64_t n_chains, int32_t dim,
                                    int32_t n_mh, int32_t n_leapfrog, float eps, const float* eps_table,
                                    int32_t mass_kind, double mass_scalar, const float* mass_diag, int32_t thin,
                                    float* traj, uint8_t* accept_mask, uint32_t* accept_count,
                                    const float* p_noise, const float* u, uint64_t seed, uint64_t offset, void* stream);

/*
 * Replica-exchange (parallel tempering) Langevin: n_ladders ladders of n_replicas tempered copies of a chain, k_steps
 * Euler-Maruyama steps of every copy and the swap events between them in ONE launch (an addition to ABI 9: nothing else moved).
 *
 * State: x is the SLOT MATRIX [n_ladders * n_replicas, dim], updated in place; row c * R + r is slot r of ladder c, slot 0 the
 * target.  Slot r runs at temperature T_r (T_0 < T_1 < ...) through the two device arrays noise_coef[R] and beta[R]:
 * noise_coef[r] = (float)sqrt(2 sigma^2 T_r), beta[r] = (float)(1 / (sigma^2 T_r)), formed in double on the host, rounded once.
 *
 * Step s (0 .. k_steps - 1), every slot, the reference's rounding order (as ebm_langevin_chain_f32, nothing contracted):
 *   x1 = x - eta * g;  dw = xi * sqrt_eta;  x = x1 + noise_coef[r] * dw
 * xi is the normal field at Philox step step0 + 2 s, addressed by the flat element (c * R + r) * dim + col of the slot matrix.
 *
 * Swap event m = (s + 1) / swap_every - 1 follows step s when (s + 1) % swap_every == 0.  Even m pairs the slots (0,1), (2,3), ...,
 * odd m pairs (1,2), (3,4), ...; unpaired slots do nothing.  For the pair (r, r + 1) of ladder c
 *   delta = (beta[r] - beta[r + 1]) * (E_r - E_{r+1})        raw fp32 energies of the current states, no clamp
 * and the two states change slots iff delta == delta and u < exp(min(delta, 0)) (a NaN delta rejects).  u is the uniform field
 * (what ebm_noise_fill_f32 materialises with EBM_NOISE_UNIFORM, the field the HMC accept step reads) at Philox step
 * step0 + 2 s + 1, element c * R + r: the lower slot's row.  A call consumes the Philox steps step0 .. step0 + 2 k_steps - 1.
 *
 * After step s and its swap event, slot 0's state goes to traj[c, (s + 1) / thin - 1] whenever (s + 1) % thin == 0
 * (traj: [n_ladders, k_steps / thin, dim], or NULL).
 * swap_counts: NULL, or device uint32[2 * (R - 1)] that the call ADDS to (zero it first): attempts of the pair (p, p + 1) at
 * index p, accepted swaps at index R - 1 + p.
 * noise / u: both NULL (native draws), or the injected fields noise[k_steps, n_ladders * R, dim] and u[n_events, n_ladders * R]
 * (n_events = k_steps / swap_every; only the lower-slot entries of u are read).
 *
 * Lane-group kernels (one lane group per replica, a ladder inside one workgroup, swaps relabel the replicas and move no state):
 * every analytic energy except EBM_ENERGY_MLP (EBM_EKIND), dim <= 1024 (EBM_EDIM), 2 <= n_replicas <= 64 and
 * n_replicas * G <= 256 with G = the lanes per row, the power of two >= ceil(dim / 4), at most 64 (EBM_EDIM otherwise).
 * swap_every >= 1, thin >= 1.  Constant eta only; no diagnostics records.
 */
EBM_API int ebm_tempering_chain_f32(const ebm_energy_t* energy, float* x, int64_t n_ladders, int32_t n_replicas, int32_t dim,
                                    int32_t k_steps, float eta, float sqrt_eta, const float* noise_coef, const float* beta,
                                    int32_t swap_every, int32_t thin, float* traj, uint32_t* swap_counts, const float* noise,
                                    const float* u, uint64_t seed, uint64_t step0, void* stream);

/*
 * Replica-exchange HMC: the ladders of ebm_tempering_chain_f32 with a Metropolis-corrected HMC transition in every slot instead
 * of an Euler-Maruyama step -- n_mh transitions of every slot and the swap events between them in ONE launch (an addition to
 * ABI 9: nothing else moved).  No slot carries a discretisation bias.
 *
 * State: x is the SLOT MATRIX [n_ladders * n_replicas, dim], updated in place; row c * R + r is slot r of ladder c, slot 0 the
 * target.  Slot r samples exp(-beta_r E) with the mass M = beta_r I; in the velocity variable w = p / beta_r that is the ordinary
 * leapfrog on E itself at the kinetic temperature T_r.  The host sends three device arrays of length R:
 * sqrt_temp[r] = (float)sqrt(T_r) and beta[r] = (float)(1 / T_r), formed in double and rounded once, and eps[r], the slot's step
 * size.
 *
 * Transition t (0 .. n_mh - 1), every slot:
 *   1. w = z * sqrt_temp[r]; z is the normal field at Philox step step0 + 3 t, element (c * R + r) * dim + col
 *   2. H0 = clamp(E(x), +-1e10) + clamp(0.5 sum w^2, 0, 1e10)
 *   3. n_leapfrog safe-mode leapfrog steps on E with the step size eps[r] (the force clamp +-1e6 and the NaN scrubs of
 *      ebm_hmc_chain_f32; the same carried energy and force, merged kicks and literal fallback)
 *   4. H1 the same way from the proposal
 *   5. d = clamp(beta[r] * (H0 - H1), +-50), a = min(1, exp d)
 *   6. the proposal is accepted iff u < a; u is the uniform field at step step0 + 3 t + 1, element c * R + r.  A NaN rejects.
 *
 * Swap event m = (t + 1) / swap_every - 1 follows transition t when (t + 1) % swap_every == 0; the pairing by the parity of m
 * and the rule are those of ebm_tempering_chain_f32: delta = (beta[r] - beta[r + 1]) * (E_r - E_{r+1}) on the raw fp32 energies
 * of the states the slots now hold (an accepted proposal's E1, else E0: the energies the transitions carry -- an event evaluates
 * nothing), and the pair swaps iff delta == delta and u < exp(min(delta, 0)), u the uniform field at step step0 + 3 t + 2,
 * element c * R + r: the lower slot's row.  Nothing a state carries (x, E(x), the force) depends on the temperature, so a swap
 * exchanges the labels: slot index, eps, sqrt_temp, beta.  A call consumes the Philox steps step0 .. step0 + 3 n_mh - 1.
 *
 * After transition t and its event, slot 0's state goes to traj[c, (t + 1) / thin - 1] whenever (t + 1) % thin == 0
 * (traj: [n_ladders, n_mh / thin, dim], or NULL).
 * accept_mask: NULL, or uint8[n_mh, n_ladders * R] indexed by slot row (1 = the slot's proposal was accepted).
 * accept_counts: NULL, or device uint32[R] the call ADDS to: accepted proposals per slot over the call (n_mh * n_ladders were
 * proposed in each).  swap_counts: NULL, or device uint32[2 * (R - 1)] the call ADDS to, as in ebm_tempering_chain_f32.
 * p_noise / u_accept / u_swap: all three NULL (native draws) or all three given: p_noise[n_mh, n_ladders * R, dim],
 * u_accept[n_mh, n_ladders * R], u_swap[n_events, n_ladders * R] (n_events = n_mh / swap_every; lower-slot entries are read).
 *
 * Consequences: with beta = sqrt_temp = 1 in every slot and no event, the rows are ebm_hmc_chain_f32 chains (identity mass) on
 * the lane-group kernel of the same geometry, bit for bit.  On a quadratic energy one step size gives every slot the same
 * acceptance (the trajectory scales with sqrt(T) and beta undoes it in d); eps[R] exists for quartic walls and the like, where
 * a hot slot needs a shorter step.
 *
 * Lane-group kernels (one lane group per walker, one vector per lane): identity mass; every analytic energy except EBM_ENERGY_MLP
 * (EBM_EKIND); dim <= 256 (EBM_EDIM); 2 <= n_replicas <= 64 and n_replicas * G <= 256 with G = the lanes per row, the power of
 * two >= ceil(dim / 4) (EBM_EDIM otherwise).  swap_every >= 1, thin >= 1, n_leapfrog >= 1.  Constant step sizes only; no
 * diagnostics records.
 */
EBM_API int ebm_tempering_hmc_chain_f32(const ebm_energy_t* energy, float* x, int64_t n_ladders, int32_t n_replicas, int32_t dim,
                                        int32_t n_mh, int32_t n_leapfrog, const float* eps, const float* sqrt_temp,
                                        const float* beta, int32_t swap_every, int32_t thin, float* traj, uint8_t* accept_mask,
                                        uint32_t* accept_counts, uint32_t* swap_counts, const float* p_noise,
                                        const float* u_accept, const float* u_swap, uint64_t seed, uint64_t step0, void* stream);

/*
 * Replica-exchange HMC on the MLP energy: the algorithm, the parameter list, the slot matrix (row c * R + r, slot 0 the target),
 * the Philox coordinates, the outputs and the counters of ebm_tempering_hmc_chain_f32 for EBM_ENERGY_MLP -- n_mh transitions of
 * every slot and the swap events between them in ONE launch around the matrix-core evaluation (an addition to ABI 9: nothing else
 * moved; ebm_tempering_hmc_chain_f32 keeps refusing the MLP).  docs/design/tempering_hmc_mlp.md.
 *
 * Transition t (0 .. n_mh - 1), every slot r of every ladder c:
 *     w  = sqrt_temp[r] * z                 z: the normal field at step step0 + 3 t, element (c * R + r) * dim + col
 *     E0, g = the evaluation at the held x;  f = clamp(-g, +-1e6);  H0 = clamp(E0, +-1e10) + clamp(0.5 sum w^2, 0, 1e10)
 *     n_leapfrog times:  w = fma(eps[r] / 2, f, w);  x' = fma(eps[r], w, x');  E', g' = the evaluation at x';
 *                        f = clamp(-g', +-1e6);  w = fma(eps[r] / 2, f, w)     -- the two half kicks are never merged
 *         (where E' or g' is not finite in some row of the wave: the NaN-propagating clamp, w and x' scrubbed with
 *          nan_to_num(nan = 0), and E', f re-evaluated on the scrubbed x' -- the literal safe-mode step, as in
 *          ebm_ghmc_mlp_chain_f32)
 *     H1 = clamp(E1, +-1e10) + clamp(0.5 sum w^2, 0, 1e10),  E1 = E' of the last step
 *     d  = clamp(beta[r] * (H0 - H1), +-50);  accepted iff u < min(1, exp d)   u: the uniform field at step step0 + 3 t + 1,
 *                                                                              element c * R + r; a NaN rejects
 *     e_now = accepted ? E1 : E0            raw fp32, not clamped: the energy of the state the slot now holds
 * A transition makes n_leapfrog + 1 evaluations and carries no energy, force or momentum to the next one; x lives in the
 * caller's buffer between transitions.
 *
 * Swap event m = (t + 1) / swap_every - 1 after transition t when (t + 1) % swap_every == 0: even events pair (0,1), (2,3), ..,
 * odd events (1,2), (3,4), ..; delta = (beta[r] - beta[r + 1]) * (e_now[r] - e_now[r + 1]); the pair swaps iff delta == delta and
 * u < exp(min(delta, 0)), u the uniform field at step step0 + 3 t + 2, element c * R + r, the lower slot's row.  An event
 * evaluates nothing.  A swap exchanges the two STATES (rows c * R + r and c * R + r + 1 of x).
 *
 * Outputs and draws: after the event, when (t + 1) % thin == 0, slot 0's state goes to traj[c, (t + 1) / thin - 1]
 * (traj: [n_ladders, n_mh / thin, dim] or NULL); accept_mask: NULL or uint8[n_mh, n_ladders * R] by slot row; accept_counts: NULL
 * or device uint32[R], swap_counts: NULL or device uint32[2 (R - 1)] (attempts of pair (p, p + 1) at p, accepts at R - 1 + p),
 * both ADDED to, once per workgroup at the end of the call; p_noise[n_mh, n_ladders * R, dim] / u_accept[n_mh, n_ladders * R] /
 * u_swap[n_mh / swap_every, n_ladders * R]: all three NULL or all three given.  The call owns the Philox steps
 * step0 .. step0 + 3 n_mh - 1.  Columns past dim and rows past n_ladders * R never reach memory; 64-bit row indices.
 *
 * Two calls equal one whenever the first holds an even number of events (m restarts at 0 in every call): (n1, step0) then
 * (n2, step0 + 3 n1) with n1 % (2 swap_every) == 0 gives the bits of one call of n1 + n2.  With sqrt_temp = beta = 1 in every
 * slot, one eps and no event the rows are ebm_ghmc_mlp_chain_f32 chains at gamma = inf on the same draws.
 *
 * The evaluation is three-way split bf16 (or exact-f32 MFMA) arithmetic with fp32 accumulation: fp32 accuracy, not autograd's
 * rounding.
 *
 * Refusals, all in front of any device access and of the early return for n_ladders == 0: a NULL energy, x, eps, sqrt_temp or
 * beta; n_mh, n_leapfrog, thin or swap_every below 1; n_ladders < 0; draws given in part; x, traj or p_noise not 16-byte aligned
 * (EBM_EINVAL); a kind other than EBM_ENERGY_MLP (EBM_EKIND); a hidden width (energy->n_comp) other than 64 / 128, dim outside
 * 1 .. 128 or n_replicas not in {2, 4, 8, 16, 32} (EBM_EDIM, the message names the three numbers).  No H = 256, no pre-split W1
 * image (energy->aux is ignored), no tables, no mass matrix, no diagnostics records.
 */
EBM_API int ebm_tempering_hmc_mlp_chain_f32(const ebm_energy_t* energy, float* x, int64_t n_ladders, int32_t n_replicas, int32_t dim,
                                            int32_t n_mh, int32_t n_leapfrog, const float* eps, const float* sqrt_temp,
                                            const float* beta, int32_t swap_every, int32_t thin, float* traj, uint8_t* accept_mask,
                                            uint32_t* accept_counts, uint32_t* swap_counts, const float* p_noise,
                                            const float* u_accept, const float* u_swap, uint64_t seed, uint64_t step0, void* stream);

/*
 * Replica-exchange Langevin on the MLP energy: the algorithm, the parameter list, the slot matrix (row c * R + r, slot 0 the
 * target), the Philox coordinates, the outputs and the counters of ebm_tempering_chain_f32 for EBM_ENERGY_MLP -- k_steps
 * Euler-Maruyama steps of every slot and the swap events between them in ONE launch around the matrix-core evaluation (an addition
 * to ABI 9: nothing else moved; ebm_tempering_chain_f32 keeps refusing the MLP).  docs/design/tempering_mlp.md.
 *
 * Step s (0 .. k_steps - 1), every slot r of every ladder c:
 *     E, g = the evaluation at x            raw: no clamp on either, a NaN stays in its row
 *     x1 = x - eta * g;  dw = z * sqrt_eta;  x = x1 + noise_coef[r] * dw     every operation rounded on its own
 *                                           z: the normal field at step step0 + 2 s, element (c * R + r) * dim + col
 * Columns past dim are held at 0.
 *
 * Swap event m = (s + 1) / swap_every - 1 after step s when (s + 1) % swap_every == 0: even events pair (0,1), (2,3), .., odd
 * events (1,2), (3,4), ..; delta = (beta[r] - beta[r + 1]) * (E_r - E_{r+1}) on the raw fp32 energies of the states behind step
 * s; the pair swaps iff delta == delta and u < exp(min(delta, 0)), u the uniform field at step step0 + 2 s + 1, element
 * c * R + r, the lower slot's row.  A swap exchanges the two STATES (rows c * R + r and c * R + r + 1 of x).  The energies of an
 * event are those of the evaluation that yields step s + 1's gradient, made at the state behind step s; the gradient moves with
 * the state, so an event costs no evaluation: a call makes k_steps + 1 evaluations when k_steps % swap_every == 0 (the last one
 * for the last event's energies alone) and k_steps otherwise.  A kept step behind the last step with no event due there
 * evaluates nothing: the state behind step k_steps - 1 is stored as it stands.
 *
 * Outputs and draws: after step s and its event, when (s + 1) % thin == 0, slot 0's state goes to traj[c, (s + 1) / thin - 1]
 * (traj: [n_ladders, k_steps / thin, dim] or NULL); swap_counts: NULL or device uint32[2 (R - 1)] (attempts of pair (p, p + 1) at
 * p, accepts at R - 1 + p), ADDED to, once per workgroup at the end of the call; noise[k_steps, n_ladders * R, dim] /
 * u[k_steps / swap_every, n_ladders * R]: both NULL (native draws) or both given (only the lower-slot entries of u are read;
 * with no event in the call u is not read).  The call owns the Philox steps step0 .. step0 + 2 k_steps - 1.
 * x is read once and written once, at the end of the call; columns past dim and rows past n_ladders * R never reach memory;
 * 64-bit row indices.
 *
 * Two calls equal one whenever the first holds an even number of events (m restarts at 0 in every call): (n1, step0) then
 * (n2, step0 + 2 n1) with n1 % (2 swap_every) == 0 gives the bits of one call of n1 + n2 -- the first call's last evaluation and
 * the second call's first are the same function of the same rows.  With no event in the call, slot r's rows are
 * ebm_chain_moments_mlp_f32 chains at noise_coef[r] on the same draws, bit for bit.
 *
 * The evaluation is three-way split bf16 (or exact-f32 MFMA) arithmetic with fp32 accumulation: fp32 accuracy, not autograd's
 * rounding.
 *
 * Refusals, all in front of any device access and of the early return for n_ladders == 0: a NULL energy, x, noise_coef or beta;
 * k_steps, thin or swap_every below 1; n_ladders < 0; draws given in part; eta or sqrt_eta NaN or infinite; x, traj or noise not
 * 16-byte aligned (EBM_EINVAL); a kind other than EBM_ENERGY_MLP (EBM_EKIND); a hidden width (energy->n_comp) other than
 * 64 / 128, dim outside 1 .. 128 or n_replicas not in {2, 4, 8, 16, 32} (EBM_EDIM, the message names the three numbers).  No
 * H = 256, no pre-split W1 image (energy->aux is ignored), no tables, no clamp, no diagnostics records.
 */
EBM_API int ebm_tempering_mlp_chain_f32(const ebm_energy_t* energy, float* x, int64_t n_ladders, int32_t n_replicas, int32_t dim,
                                        int32_t k_steps, float eta, float sqrt_eta, const float* noise_coef, const float* beta,
                                        int32_t swap_every, int32_t thin, float* traj, uint32_t* swap_counts, const float* noise,
                                        const float* u, uint64_t seed, uint64_t step0, void* stream);

/*
 * Annealed importance sampling (Neal 2001): every chain walks ONE state from the base N(0, sigma0^2 I) to the target through
 * n_temps tempered laws and accumulates the importance weight whose mean estimates Z / Z_0 -- the whole walk in ONE launch (an
 * addition to ABI 9: nothing else moved).  The third member of the tempered family: the replica-exchange entries run R
 * temperatures side by side, this one runs T = n_temps of them in time.
 *
 * Base and path: E_0(x) = 0.5 * inv_var0 * sum x^2 (log Z_0 = dim / 2 * log(2 pi sigma0^2)), U_b(x) = (1 - b) E_0(x) + b E(x).
 * beta: device float[T + 1], beta[0] = 0, beta[T] = 1, non-decreasing; eps: device float[T], the step size of transition t at
 * eps[t - 1].  The host forms the schedule in double and rounds once; sigma0 = (float)sigma_0, inv_var0 = (float)(1 / sigma_0^2).
 *
 * Start: x = sigma0 * z, z the normal field at Philox step step0, element chain * dim + col -- or the injected x0[n, dim];
 * logw = 0.
 * Step t = 1 .. T, every chain:
 *   1. logw += (beta[t] - beta[t - 1]) * (E_0(x) - E(x)): difference and product in fp32, on the energies of the state the
 *      chain holds (carried from the previous transition: the update evaluates nothing); the running sum is a compensated
 *      (Kahan) fp32 pair per chain.
 *   2. one Metropolis-corrected HMC transition that leaves exp(-U_{beta[t]}) invariant: identity mass, n_leapfrog safe-mode
 *      leapfrog steps of size eps[t - 1] with the force clamp(-((1 - b) inv_var0 x + b dE/dx), +-1e6) (the NaN scrubs, merged
 *      kicks and literal fallback of ebm_hmc_chain_f32), H = clamp(U, +-1e10) + clamp(0.5 sum p^2, 0, 1e10),
 *      d = clamp(H0 - H1, +-50), accepted iff u < min(1, exp d); a NaN rejects.  The momentum is the normal field at step
 *      step0 + 2 t - 1, element chain * dim + col; u the uniform field at step step0 + 2 t, element chain.
 * A call consumes the Philox steps step0 .. step0 + 2 T.
 *
 * Out: logw[n]; x[n, dim], the final states (written once, never read: approximately target samples that carry the weights).
 * accept_mask: NULL, or uint8[T, n] (row t - 1: transition t).  accept_counts: NULL, or device uint32[T] the call ADDS to:
 * accepted proposals of each temperature (n were proposed at each) -- what eps[t] is tuned with.
 * x0 / p_noise / u_accept: all three NULL (native draws) or all three given: x0[n, dim], p_noise[T, n, dim], u_accept[T, n].
 *
 * Consequence: the mix is formed as (1 - b) * a + b * c, never divided by b, so at b = 1 the transition is ebm_hmc_chain_f32's
 * on the lane-group kernel of the same geometry, bit for bit (finite states).
 *
 * Lane-group kernels (one lane group per chain, one vector per lane, no exchange between chains): every analytic energy except
 * EBM_ENERGY_MLP (EBM_EKIND); dim <= 256 (EBM_EDIM, in front of any device access); n_temps >= 1, n_leapfrog >= 1.
 */
EBM_API int ebm_ais_chain_f32(const ebm_energy_t* energy, float* x, float* logw, int64_t n_chains, int32_t dim, int32_t n_temps,
                              int32_t n_leapfrog, const float* beta, const float* eps, float sigma0, float inv_var0,
                              uint8_t* accept_mask, uint32_t* accept_counts, const float* x0, const float* p_noise,
                              const float* u_accept, uint64_t seed, uint64_t step0, void* stream);

/*
 * Annealed importance sampling on EBM_ENERGY_MLP -- the energy the package trains -- in ONE launch (an addition to ABI 9:
 * nothing else moved; ebm_ais_chain_f32 keeps refusing the MLP).  Parameters, base, path, draws and outputs are exactly those of
 * ebm_ais_chain_f32 above; what differs is where the energies of step 1 come from:
 *
 * Start: x = sigma0 * z, z the normal field at Philox step step0, element chain * dim + col -- or the injected x0[n, dim];
 * logw = 0.
 * Step t = 1 .. T, every chain, with db = beta[t] - beta[t - 1], b = beta[t], b0 = 1 - b, c0 = b0 * inv_var0 formed in fp32:
 *   1. ONE evaluation at the held state gives E(x) and dE/dx; E_0(x) = 0.5 * inv_var0 * sum x^2.
 *      logw += db * (E_0 - E), the running sum a compensated (Kahan) fp32 pair per chain; an infinite sum stays what a plain
 *      sum gives.
 *   2. one Metropolis-corrected HMC transition that leaves exp(-U_b) invariant: identity mass, momentum the normal field at
 *      step step0 + 2 t - 1, H0 = clamp(b0 * E_0 + b * E, +-1e10) + clamp(0.5 sum p^2, 0, 1e10), the first force
 *      clamp(-(c0 * x + b * dE/dx), +-1e6) from the evaluation of 1., n_leapfrog safe-mode leapfrog steps of size eps[t - 1]
 *      (one evaluation each: the same mix of its gradient is the next force; NaN scrubs, merged kicks and literal fallback of
 *      ebm_hmc_chain_f32), H1 from U = b0 * E_0(x') + b * E(x'), d = clamp(H0 - H1, +-50), accepted iff u < min(1, exp d), u the
 *      uniform field at step step0 + 2 t, element chain; a NaN rejects.
 * A transition costs n_leapfrog + 1 evaluations, as ebm_hmc_chain_f32's on this energy.  A call consumes the Philox steps
 * step0 .. step0 + 2 T.
 *
 * The evaluation is the matrix-core one of ebm_hmc_chain_f32 / ebm_energy_grad_f32 (three-way split bf16 operands or exact-f32
 * MFMA, fp32 accumulation): fp32 accuracy, not autograd's rounding.  One wave walks 32 chains.
 * x is output only: the kernel keeps the held state there between transitions and never reads a word it has not written.
 *
 * Consequence: at b = 1 the mix is 0 * a + 1 * c = c, and the transition is ebm_hmc_chain_f32's on this energy with the same
 * injected draws (identity mass), bit for bit (finite states).
 *
 * Refusals, all in front of any device access: a NULL energy, x, logw, beta or eps, n_temps < 1, n_leapfrog < 1, or x0 /
 * p_noise / u_accept not given together (EBM_EINVAL); a kind other than EBM_ENERGY_MLP (EBM_EKIND); a hidden width
 * (energy->n_comp) other than 64 / 128 or dim outside 1 .. 128 (EBM_EDIM).  Identity mass only; no trajectory, no thinning, no
 * diagnostics records; no H = 256, no pre-split W1 image (energy->aux is ignored).
 */
EBM_API int ebm_ais_mlp_chain_f32(const ebm_energy_t* energy, float* x, float* logw, int64_t n_chains, int32_t dim, int32_t n_temps,
                                  int32_t n_leapfrog, const float* beta, const float* eps, float sigma0, float inv_var0,
                                  uint8_t* accept_mask, uint32_t* accept_counts, const float* x0, const float* p_noise,
                                  const float* u_accept, uint64_t seed, uint64_t step0, void* stream);

/*
 * Per-chain running moments: k_steps transitions of a Langevin (sampler = 0) or HMC (sampler = 1) walker per chain that keeps,
 * beside its state, the time average and the sum of squared deviations of every coordinate -- and of the energy -- over two
 * halves of the counted steps, in ONE launch (an addition to ABI 9: nothing else moved).  From them the host forms split-R-hat,
 * a between-sequence effective sample size and burn-in-aware posterior means (torchebm_amd/samplers/moments.py) without a
 * trajectory: the extra traffic is four state-sized planes per launch, whatever k_steps is.
 *
 * Counted states.  The first burn_in transitions are not counted; the remaining 2 h are counted as two halves of h states each.
 * k_steps - burn_in == 2 h and h >= 2 are required (EBM_EINVAL before any launch).  A counted state is the state AFTER the
 * transition; for HMC a rejected proposal counts the held state again.
 *
 * Accumulator.  Per chain, per coordinate and per half a Welford pair in fp32, every operation rounded on its own; with
 * c = 1 .. h the count within the half and x the counted value:
 *     d = x - mean;   mean = mean + d * recip[c - 1];   M2 = M2 + d * (x - mean)
 * recip: device float[h], recip[c - 1] = (float)(1.0 / c) formed in double and rounded once (a wave-uniform load per step; the
 * kernel divides nothing).  Both start from zero: c = 1 gives mean = x and M2 = 0 with no special first step.
 *
 * Outputs.
 *   mom     float[4][n_chains][dim]: the planes mean_a, M2_a, mean_b, M2_b (a = first half), written once at the end.
 *   e_mom   NULL, or float[4][n_chains]: the same four quantities for the energy E(x) of the counted states, the value the
 *           kind's evaluation returns, unclamped.  HMC: the energy the transition carries (no evaluation).  Langevin: the
 *           evaluation at the top of the next step returns energy and gradient together, plus one evaluation behind the last
 *           step; with e_mom == NULL the Langevin kernel is another instantiation that carries no group reduction.
 *   x       in/out, the final states.
 *   traj    NULL, or float[n_chains][2 h][dim]: the counted states; e_traj: NULL, or float[n_chains][2 h]: their energies
 *           (Langevin: written only when e_mom is given).  For tests and small runs.
 *   accept_mask / accept_count (HMC; ignored for Langevin): NULL, or uint8[k_steps][n_chains] / device uint32[k_steps] the call
 *           ADDS to, as in ebm_hmc_chain_f32.
 * Slots of a lane that hold no column never reach memory.
 *
 * Langevin transition (eta, sqrt_eta, noise_coef: constants): x' = (x - eta * dE/dx) + noise_coef * (z * sqrt_eta), every
 * operation rounded on its own, in the reference's order (ebm_langevin_chain_f32 without clamp).  z is the normal field at
 * Philox step offset + s, element chain * dim + col -- ebm_langevin_chain_f32's coordinates, so for the element-wise energies
 * the final states equal that entry's bit for bit -- or the injected noise_or_p[k_steps, n_chains, dim].  u is ignored.
 *
 * HMC transition (n_leapfrog, eps: constants): ebm_hmc_chain_f32's on the lane-group kernel of the same geometry: identity
 * mass, n_leapfrog safe-mode leapfrog steps; energy and force carried from the accepted state, the start's from the
 * pseudo-transition.  Momentum: the normal field at step offset + 2 t, the accept uniform at offset + 2 t + 1, element chain
 * -- or injected noise_or_p[k_steps, n_chains, dim] and u[k_steps, n_chains], both or neither (EBM_EINVAL).
 *
 * Limits: every analytic energy except EBM_ENERGY_MLP (EBM_EKIND); dim <= 256, one vector per lane (EBM_EDIM, in front of any
 * device access); constant coefficients, no clamp, no tables, identity mass; 64-bit row indices.  A NULL mom or recip is
 * EBM_EINVAL.
 */
EBM_API int ebm_chain_moments_f32(const ebm_energy_t* energy, float* x, int64_t n_chains, int32_t dim, int32_t sampler,
                                  int32_t k_steps, int32_t burn_in, float eta, float sqrt_eta, float noise_coef,
                                  int32_t n_leapfrog, float eps, const float* recip, float* mom, float* e_mom, float* traj,
                                  float* e_traj, uint8_t* accept_mask, uint32_t* accept_count, const float* noise_or_p,
                                  const float* u, uint64_t seed, uint64_t offset, void* stream);

/*
 * Per-chain running moments of Langevin dynamics on the MLP energy: the statistics of ebm_chain_moments_f32 above -- the same
 * parameter list, the same counted states, recip table, Welford recurrence and layouts of mom, e_mom, traj and e_traj -- around
 * the Euler-Maruyama walk on the matrix-core evaluation of the MLP, in ONE launch (an addition to ABI 9: nothing else moved;
 * ebm_chain_moments_f32 still refuses the MLP).  One wave walks 32 chains.  sampler must be 0; n_leapfrog, eps, accept_mask,
 * accept_count and u are ignored (HMC on the MLP with running moments: ebm_kinetic_moments_mlp_f32, generalized HMC at infinite
 * friction).
 *
 * Transition (eta, sqrt_eta, noise_coef: constants): ebm_langevin_chain_f32's update without clamp,
 *     x1 = x - eta * dE/dx;   dw = z * sqrt_eta;   x' = x1 + noise_coef * dw
 * every operation rounded on its own.  The gradient is raw: a NaN stays in its chain.  z is the normal field at Philox step
 * offset + s, element chain * dim + col -- the coordinates ebm_langevin_chain_f32 draws at -- or the injected
 * noise[k_steps, n_chains, dim].  A call owns the steps offset .. offset + k_steps - 1.  The gradient comes from the general
 * evaluation of the MLP walks, not from the specialised Langevin chain kernels: the final x is ebm_langevin_chain_f32's draw for
 * draw and operation for operation in the update, but not guaranteed bit for bit.
 *
 * Counted states.  The first burn_in steps are not counted; k_steps - burn_in == 2 h with h >= 2; a counted state is the state
 * AFTER the step.  Per coordinate, per half and with c = 1 .. h
 *     d = x - mean;   mean = mean + d * recip[c - 1];   M2 = M2 + d * (x - mean)
 * in fp32, every operation rounded on its own; mom is float[4][n_chains][dim] (mean_a, M2_a, mean_b, M2_b), e_mom NULL or
 * float[4][n_chains].  traj: NULL, or float[n_chains][2 h][dim], the counted states; e_traj: NULL, or float[n_chains][2 h],
 * their energies (written with or without e_mom).
 *
 * Energies add at most one evaluation.  Evaluation i >= 1 is made at the state behind step i - 1, the counted state.  With
 * e_mom or e_traj given the launch makes k_steps + 1 evaluations; with both NULL exactly k_steps: nothing is evaluated behind
 * the last step.  The value counted is the unclamped one.
 *
 * Working storage.  The pairs do not live in registers: mom and e_mom are WORKING STORAGE during the launch -- each counted step
 * reads a chain's pair from them and writes it back (a lane reads only what it stored itself) -- and defined at return.  At
 * c == 1 the pair starts from zero and the planes are not read: the caller need not initialise them, and whatever they held (a
 * NaN included) never reaches the output.  They must not overlap each other or any other buffer of the call.  Columns past
 * dim and rows past n_chains never reach memory; 64-bit row indices.
 *
 * The evaluation is three-way split bf16 (or exact-f32 MFMA) arithmetic with fp32 accumulation: fp32 accuracy, not autograd's
 * rounding.
 *
 * Refusals, all in front of any device access and of the early return for n_chains == 0.  EBM_EINVAL: a NULL energy, x, mom or
 * recip; n_chains < 0; sampler != 0; burn_in < 0 or k_steps - burn_in not 2 h with h >= 2; eta, sqrt_eta or noise_coef NaN or
 * infinite.  EBM_EKIND: a kind other than EBM_ENERGY_MLP.  EBM_EDIM: a hidden width (energy->n_comp) other than 64 / 128 or
 * dim outside 1 .. 128 (the message names both).  x, mom, traj and noise must be 16-byte aligned.  No H = 256, no pre-split W1
 * image (energy->aux is ignored), no tables, no clamp, no Heun.
 */
EBM_API int ebm_chain_moments_mlp_f32(const ebm_energy_t* energy, float* x, int64_t n_chains, int32_t dim, int32_t sampler,
                                      int32_t k_steps, int32_t burn_in, float eta, float sqrt_eta, float noise_coef,
                                      int32_t n_leapfrog, float eps, const float* recip, float* mom, float* e_mom, float* traj,
                                      float* e_traj, uint8_t* accept_mask, uint32_t* accept_count, const float* noise_or_p,
                                      const float* u, uint64_t seed, uint64_t offset, void* stream);

/*
 * Underdamped (kinetic) Langevin dynamics in the BAOAB splitting (Leimkuhler & Matthews 2013): k_steps transitions of a walker
 * per chain that carries a velocity beside its position, in ONE launch (an addition to ABI 9: nothing else moved).  Unit mass,
 * friction gamma > 0, temperature T > 0 (the target is exp(-E / T)), step h > 0.  One gradient evaluation per step, as
 * Euler-Maruyama; on a quadratic energy the position marginal is exact for every stable h (var(v) = T (1 - h^2 k / 4)).
 *
 * Constants.  The entry forms them in double and rounds each once to fp32:
 *     hh = h / 2;   c1 = exp(-gamma h);   c2 = sqrt(T * (-expm1(-2 gamma h)));   sqrt_temp = sqrt(T)
 *
 * Recurrence.  A chain carries x, v and g = dE/dx(x): the raw gradient of the kind's evaluation, no clamp (a NaN propagates
 * and stays in its chain).  The start's gradient comes from one evaluation in front of the loop.  Step s = 0 .. k_steps - 1,
 * every operation rounded on its own:
 *     v = v - hh * g            (B)
 *     x = x + hh * v            (A)
 *     v = c1 * v + c2 * z       (O)
 *     x = x + hh * v            (A)
 *     g = dE/dx(x)
 *     v = v - hh * g            (B)
 * z is the normal field at Philox step offset + 1 + s, element chain * dim + col -- or the injected noise[k_steps, n_chains,
 * dim].  The closing kick of a step and the opening kick of the next are NOT merged: the bits do not depend on where a run is
 * cut, so (k1, offset) then (k2, offset + k1) with draw_v0 = 0 equals one call of k1 + k2.
 *
 * Start velocity.  draw_v0 != 0: v is output only and the walk starts from sqrt_temp * z0, z0 the normal field at step offset
 * (also when noise is injected).  draw_v0 == 0: v is read -- velocities that persist across calls.  A call owns the Philox
 * steps offset .. offset + k_steps either way.
 *
 * Outputs.  x and v are updated in place and stored once.  traj: NULL, or float[n_chains][k_steps / thin][dim], the position
 * after step s whenever (s + 1) % thin == 0.  Slots of a lane that hold no column never reach memory.
 *
 * Limits: every analytic energy except EBM_ENERGY_MLP (EBM_EKIND); 1 <= dim <= 256, one vector per lane (EBM_EDIM, in front
 * of any device access); constants only: no clamp, no tables, unit mass (a scalar or diagonal mass:
 * ebm_kinetic_chain_mass_f32 below; no dense mass), no diagnostics records; 64-bit row indices.
 * EBM_EINVAL with no buffer touched: a NULL energy, x or v; k_steps < 1; thin < 1; h, gamma or temperature not positive.
 */
EBM_API int ebm_kinetic_chain_f32(const ebm_energy_t* energy, float* x, float* v, int64_t n_chains, int32_t dim,
                                  int32_t k_steps, double h, double gamma, double temperature, int32_t draw_v0, int32_t thin,
                                  float* traj, const float* noise, uint64_t seed, uint64_t offset, void* stream);

/*
 * The two velocity-carrying samplers with a scalar or diagonal mass: ebm_kinetic_chain_mass_f32 (here) and
 * ebm_ghmc_chain_mass_f32 (behind ebm_ghmc_chain_f32) take the parameter lists of ebm_kinetic_chain_f32 / ebm_ghmc_chain_f32
 * with `int32_t mass_kind, double mass_scalar, const float* mass_diag` directly behind `temperature`, each in ONE launch
 * (additions to ABI 9: nothing else moved).  The rules both share:
 *
 * Mass forms and clamps: those of ebm_hmc_chain_f32.  EBM_MASS_SCALAR: m_raw = (float)m, m_sqrt = (float)sqrt(m), m_safe =
 * (float)max(m, 1e-10), formed in double and rounded once.  EBM_MASS_DIAG: mass_diag is a device float[dim]; per element m_raw
 * = m, m_sqrt = sqrtf(m) (correctly rounded), m_safe = (m < 1e-10) ? 1e-10 : m.  The entries are not inspected.  A slot of a
 * lane that holds no column of the diagonal gets mass 1; x and p stay 0 there.
 *
 * Carried plane: the MOMENTUM p with law N(0, T m), the convention of ebm_hmc_chain_f32.  `v` in the parameter list is that
 * plane, in and out.  draw_v0 != 0: p = (sqrt_temp * m_sqrt) * z0, z0 the normal field at step offset.
 *
 * Unchanged from the unit-mass entries: the constants formed in double, the Philox coordinates and the steps a call owns,
 * draw_v0, thin / traj, the injected noise / u, the outputs, "two calls equal one", 1 <= dim <= 256 (EBM_EDIM), the refusal
 * of EBM_ENERGY_MLP (EBM_EKIND) and every EBM_EINVAL.  More EBM_EINVAL, in front of any device access and of the early
 * return for n_chains == 0, no buffer touched: mass_kind == EBM_MASS_NONE or unknown (callers use the unit-mass entry);
 * EBM_MASS_DIAG with a NULL mass_diag; EBM_MASS_SCALAR with a mass_scalar that is not positive and finite.
 *
 * BAOAB with a mass.  a_j = hh / m_safe_j and s_j = c2 * m_sqrt_j are formed once per coordinate in front of the loop; step
 * s = 0 .. k_steps - 1, every operation rounded on its own, g the raw unclamped gradient:
 *     p = p - hh * g            (B)
 *     x = x + a_j * p           (A)
 *     p = c1 * p + s_j * z      (O)
 *     x = x + a_j * p           (A)
 *     g = dE/dx(x)
 *     p = p - hh * g            (B)
 * With every m_j = 1 each line is ebm_kinetic_chain_f32's with an exact factor: the bits are that entry's.  On a quadratic
 * energy E'' = k the law is the unit-mass one in the coordinate x sqrt(m): var(x) k / T = 1, var(p) / (T m) = 1 - h^2 k / (4 m).
 */
EBM_API int ebm_kinetic_chain_mass_f32(const ebm_energy_t* energy, float* x, float* v, int64_t n_chains, int32_t dim,
                                       int32_t k_steps, double h, double gamma, double temperature, int32_t mass_kind,
                                       double mass_scalar, const float* mass_diag, int32_t draw_v0, int32_t thin, float* traj,
                                       const float* noise, uint64_t seed, uint64_t offset, void* stream);

/*
 * Underdamped Langevin (BAOAB) on the MLP energy: the walk of ebm_kinetic_chain_f32 above -- the same parameter list, the same
 * constants formed in double and rounded once, the same Philox coordinates -- with the matrix-core evaluation of
 * ebm_hmc_chain_f32 / ebm_ais_mlp_chain_f32 inside the step loop, in ONE launch (an addition to ABI 9: nothing else moved;
 * ebm_kinetic_chain_f32 still refuses the MLP).  One wave walks 32 chains; only the gradient is evaluated, never the energy.
 *
 * Recurrence.  The contract above restated for a loop with ONE evaluation site: k_steps + 1 evaluations i = 0 .. k_steps, every
 * product and sum rounded on its own, the raw gradient unclamped (a NaN stays in its chain):
 *     g = dE/dx(x)
 *     if i > 0:  v = v - hh * g             (the closing B of step i - 1; then x goes to traj if i % thin == 0)
 *     if i == k_steps: stop
 *     v = v - hh * g                        (the opening B: never merged with the closing one)
 *     x = x + hh * v                        (A)
 *     v = c1 * v + c2 * z_i                 (O)
 *     x = x + hh * v                        (A)
 * z_i is the normal field at Philox step offset + 1 + i, element chain * dim + col -- or the injected noise[k_steps, n_chains,
 * dim].  draw_v0 != 0: v is output only and starts as sqrt_temp * z, z the field at step offset; draw_v0 == 0: v is read.  A
 * call owns the steps offset .. offset + k_steps.  (k1, offset) then (k2, offset + k1) with draw_v0 = 0 equals one call of
 * k1 + k2 bit for bit: the evaluation the second call starts with is the one the first call's last closing B used.
 *
 * Outputs.  x and v are updated in place and stored once; traj: NULL, or float[n_chains][k_steps / thin][dim].  Columns past
 * dim never reach memory; 64-bit row indices.
 *
 * The evaluation is three-way split bf16 (or exact-f32 MFMA) arithmetic with fp32 accumulation: fp32 accuracy, not autograd's
 * rounding.
 *
 * Refusals, all in front of any device access and of the early return for n_chains == 0: a NULL energy, x or v, k_steps < 1,
 * thin < 1, h, gamma or temperature not positive and finite (EBM_EINVAL); a kind other than EBM_ENERGY_MLP (EBM_EKIND); a
 * hidden width (energy->n_comp) other than 64 / 128 or dim outside 1 .. 128 (EBM_EDIM).  No H = 256, no pre-split W1 image
 * (energy->aux is ignored), no clamp, no tables, unit mass (a scalar or diagonal mass: ebm_kinetic_mlp_chain_mass_f32,
 * ebm_hip_mass_mlp.h), no diagnostics records.
 */
EBM_API int ebm_kinetic_mlp_chain_f32(const ebm_energy_t* energy, float* x, float* v, int64_t n_chains, int32_t dim,
                                      int32_t k_steps, double h, double gamma, double temperature, int32_t draw_v0,
                                      int32_t thin, float* traj, const float* noise, uint64_t seed, uint64_t offset,
                                      void* stream);

/*
 * Generalized HMC (Horowitz 1991; Metropolis-adjusted kinetic Langevin): n_mh transitions of a walker per chain that carries a
 * velocity beside its position, in ONE launch (an addition to ABI 9: nothing else moved).  Each transition refreshes the
 * velocity partially, runs a short Metropolis-corrected leapfrog trajectory and flips the velocity on a reject: exp(-E / T) is
 * sampled exactly for every step size, as by ebm_hmc_chain_f32, and with weak friction the walker keeps its direction across
 * transitions, as ebm_kinetic_chain_f32's does.  Unit mass, step eps > 0, n_leapfrog = L >= 1 steps, friction gamma > 0 (+inf
 * allowed), temperature T > 0 (beta = 1 / T).
 *
 * Constants.  The entry forms them in double and rounds each once to fp32 (eps itself too):
 *     c1 = exp(-gamma eps L);   c2 = sqrt(T * (-expm1(-2 gamma eps L)));   sqrt_temp = sqrt(T);   beta = 1 / T
 * gamma = +inf gives c1 = 0 and c2 = sqrt_temp exactly: a full refresh, the transition of ebm_hmc_chain_f32.
 *
 * A chain carries x, v, E(x) and the clamped force at x from the load to the one store; the last two come from the
 * pseudo-transition of ebm_hmc_chain_f32's lane-group kernel (one evaluation in front of the first transition).
 * Transition t = 0 .. n_mh - 1:
 *     v  = c1 * v + c2 * z_t                       (O)  two products and a sum, each rounded on its own
 *     u  = the uniform of this chain
 *     H0 = clamp(E(x), +-1e10) + clamp(0.5 sum v^2, 0, 1e10)
 *     (x', v') = n_leapfrog safe-mode leapfrog steps of size eps from (x, v): the trajectory of ebm_hmc_chain_f32, identity
 *                mass (the force clamp +-1e6, the NaN scrubs, the carried energy and force, merged kicks, literal fallback)
 *     H1 = clamp(E(x'), +-1e10) + clamp(0.5 sum v'^2, 0, 1e10)
 *     d  = clamp(beta * (H0 - H1), +-50);  a = min(1, exp d);  accepted iff u < a (a NaN rejects)
 *     accepted:  (x, v, E, force) = (x', v', E', force')
 *     rejected:  x, E and the force stay;  v = -(the v after O)                                  the flip
 *
 * Draws.  A call owns the Philox steps offset .. offset + 2 n_mh.  z_t is the normal field at step offset + 1 + 2 t, element
 * chain * dim + col; u the uniform field at step offset + 2 + 2 t, element chain.  draw_v0 != 0: v is output only and the walk
 * starts from sqrt_temp * z, z the normal field at step offset (also when draws are injected); draw_v0 == 0: v is read --
 * velocities that persist across calls.  noise: NULL, or float[n_mh][n_chains][dim] in place of z_t; u: NULL, or
 * float[n_mh][n_chains] in place of the uniforms; either may be given without the other.
 *
 * Outputs.  x and v are updated in place and stored once.  traj: NULL, or float[n_chains][n_mh / thin][dim], the position
 * after transition t whenever (t + 1) % thin == 0.  accept_mask: NULL, or uint8[n_mh][n_chains] (1 = accepted).  Slots of a
 * lane that hold no column never reach memory.
 *
 * Two calls equal one: (n1, offset) then (n2, offset + 2 n1) with draw_v0 = 0 produces the bits of one call of n1 + n2 -- the
 * carried energy and force are re-evaluated by the evaluation the last leapfrog step ended on.
 *
 * Limits: every analytic energy except EBM_ENERGY_MLP (EBM_EKIND); 1 <= dim <= 256, one vector per lane (EBM_EDIM, in front
 * of any device access); constants only: no tables, unit mass (a scalar or diagonal mass: ebm_ghmc_chain_mass_f32 below; no
 * dense mass), no diagnostics records; 64-bit row indices.
 * EBM_EINVAL with no buffer touched: a NULL energy, x or v; n_mh < 1, n_leapfrog < 1 or thin < 1; eps, gamma or temperature
 * not positive, or NaN (eps and temperature must be finite).  An empty call (n_chains == 0) returns 0 behind these checks.
 */
EBM_API int ebm_ghmc_chain_f32(const ebm_energy_t* energy, float* x, float* v, int64_t n_chains, int32_t dim, int32_t n_mh,
                               int32_t n_leapfrog, double eps, double gamma, double temperature, int32_t draw_v0,
                               int32_t thin, float* traj, uint8_t* accept_mask, const float* noise, const float* u,
                               uint64_t seed, uint64_t offset, void* stream);

/*
 * Generalized HMC with a scalar or diagonal mass (an addition to ABI 9: nothing else moved).  The parameter list, the mass
 * forms, the carried momentum plane, what stays as in the unit-mass entry and the refusals: the rules stated at
 * ebm_kinetic_chain_mass_f32.  s_j = c2 * m_sqrt_j and the drift scale eps / m_safe_j are formed once per coordinate in front
 * of the loop.  Transition t = 0 .. n_mh - 1:
 *     p  = c1 * p + s_j * z_t                      (O)  two products and a sum, each rounded on its own
 *     u  = the uniform of this chain
 *     H0 = clamp(E(x), +-1e10) + K_m(p),  K_m the massed kinetic energy of ebm_hmc_chain_f32: 0.5 sum(p^2 / m_raw) for a
 *          diagonal mass, (0.5 sum p^2) / m_raw for a scalar one, clamped to [0, 1e10]
 *     (x', p') = the trajectory of ebm_hmc_chain_f32 with this mass, untouched: safe mode, the drift x += (eps / m_safe) p as
 *                one FMA, the carried energy and force, the pseudo-transition, merged kicks, the literal fallback
 *     H1 = clamp(E(x'), +-1e10) + K_m(p')
 *     d  = clamp(beta * (H0 - H1), +-50);  a = min(1, exp d);  accepted iff u < a (a NaN rejects)
 *     accepted:  (x, p, E, force) = (x', p', E', force')
 *     rejected:  x, E and the force stay;  p = -(the p after O)                                  the flip
 * With every m_j = 1 the bits are ebm_ghmc_chain_f32's.  At gamma = +inf and T = 1, for finite states, this is the transition
 * of ebm_hmc_chain_f32 with the same mass on the same z and u.
 */
EBM_API int ebm_ghmc_chain_mass_f32(const ebm_energy_t* energy, float* x, float* v, int64_t n_chains, int32_t dim, int32_t n_mh,
                                    int32_t n_leapfrog, double eps, double gamma, double temperature, int32_t mass_kind,
                                    double mass_scalar, const float* mass_diag, int32_t draw_v0, int32_t thin, float* traj,
                                    uint8_t* accept_mask, const float* noise, const float* u, uint64_t seed, uint64_t offset,
                                    void* stream);

/*
 * Generalized HMC on the MLP energy: the sampler of ebm_ghmc_chain_f32 above -- the same parameter list, the same constants
 * formed in double and rounded once (c1, c2, sqrt_temp, beta, eps), the same Philox coordinates -- with the matrix-core
 * evaluation of ebm_hmc_chain_f32 / ebm_ais_mlp_chain_f32 inside the trajectory, in ONE launch (an addition to ABI 9: nothing
 * else moved; ebm_ghmc_chain_f32 still refuses the MLP).  One wave walks 32 chains.
 *
 * State.  The held x and v live in the caller's x / v buffers between transitions (a lane reads back only what it stored
 * itself); no energy and no force is carried from one transition to the next.
 *
 * Transition t = 0 .. n_mh - 1, the contract above restated for this evaluation (the transition of ebm_ais_mlp_chain_f32 at
 * beta = 1 around the refresh and the flip):
 *     v  = c1 * v + c2 * z_t                       (O)  two products and a sum, each rounded on its own; v is stored back
 *     E, g = the evaluation at the held x;  f = clamp(-g, +-1e6)
 *     H0 = clamp(E, +-1e10) + clamp(0.5 sum v^2, 0, 1e10)
 *     n_leapfrog times:  v = fma(eps / 2, f, v);  x' = fma(eps, v, x');  E', g' = the evaluation at x';
 *                        f = clamp(-g', +-1e6);  v = fma(eps / 2, f, v)       -- the two half kicks are never merged
 *         (where E' or g' is not finite in some chain of the wave: the NaN-propagating clamp, v and x' scrubbed with
 *          nan_to_num(nan = 0), and E', f re-evaluated on the scrubbed x' -- the literal safe-mode step; a NaN in v alone is
 *          scrubbed in place)
 *     H1 = clamp(E', +-1e10) + clamp(0.5 sum v^2, 0, 1e10)
 *     d  = clamp(beta * (H0 - H1), +-50);  a = min(1, exp d);  accepted iff u < a (a NaN rejects)
 *     accepted:  x = x', v = v' are stored
 *     rejected:  x stays;  v = -(the stored v after O)                                           the flip
 * A transition makes n_leapfrog + 1 evaluations.
 *
 * Draws.  A call owns the Philox steps offset .. offset + 2 n_mh.  z_t is the normal field at step offset + 1 + 2 t, element
 * chain * dim + col; u the uniform field at step offset + 2 + 2 t, element chain.  draw_v0 != 0: v is output only and the walk
 * starts from sqrt_temp * z, z the normal field at step offset (also when draws are injected); draw_v0 == 0: v is read.
 * noise: NULL, or float[n_mh][n_chains][dim] in place of z_t; u: NULL, or float[n_mh][n_chains] in place of the uniforms; either
 * may be given without the other.
 *
 * Outputs.  x and v hold the final state.  traj: NULL, or float[n_chains][n_mh / thin][dim], the held position after
 * transition t whenever (t + 1) % thin == 0.  accept_mask: NULL, or uint8[n_mh][n_chains] (1 = accepted).  Columns past dim and
 * rows past n_chains never reach memory; 64-bit row indices.
 *
 * Two calls equal one: (n1, offset) then (n2, offset + 2 n1) with draw_v0 = 0 produces the bits of one call of n1 + n2 -- nothing
 * but x and v passes from one transition to the next.
 *
 * The evaluation is three-way split bf16 (or exact-f32 MFMA) arithmetic with fp32 accumulation: fp32 accuracy, not autograd's
 * rounding.
 *
 * Refusals, all in front of any device access and of the early return for n_chains == 0: a NULL energy, x or v, n_mh < 1,
 * n_leapfrog < 1, thin < 1, n_chains < 0, eps, gamma or temperature not positive, or NaN, a non-finite eps or temperature
 * (EBM_EINVAL; gamma = +inf is allowed); a kind other than EBM_ENERGY_MLP (EBM_EKIND); a hidden width (energy->n_comp) other than
 * 64 / 128 or dim outside 1 .. 128 (EBM_EDIM, the message names both).  x, v, traj and noise must be 16-byte aligned.  No
 * H = 256, no pre-split W1 image (energy->aux is ignored), no tables, unit mass (a scalar or
 * diagonal mass: ebm_ghmc_mlp_chain_mass_f32, ebm_hip_mass_mlp.h), no diagnostics records.
 */
EBM_API int ebm_ghmc_mlp_chain_f32(const ebm_energy_t* energy, float* x, float* v, int64_t n_chains, int32_t dim, int32_t n_mh,
                                   int32_t n_leapfrog, double eps, double gamma, double temperature, int32_t draw_v0,
                                   int32_t thin, float* traj, uint8_t* accept_mask, const float* noise, const float* u,
                                   uint64_t seed, uint64_t offset, void* stream);

/*
 * Per-chain running moments of the two velocity-carrying samplers: k_steps transitions of the BAOAB walker of
 * ebm_kinetic_chain_f32 (sampler = 0) or of the generalized-HMC walker of ebm_ghmc_chain_f32 (sampler = 1) per chain that
 * keeps, beside position and velocity, the Welford pairs of ebm_chain_moments_f32 in registers, in ONE launch (an addition to
 * ABI 9: nothing else moved).  The host forms split-R-hat, a between-sequence effective sample size and pooled moments from
 * them (torchebm_amd/samplers/moments.py) without a trajectory.
 *
 * Counted states, accumulator, recip, mom, e_mom, traj, e_traj: exactly as in ebm_chain_moments_f32.  The first burn_in
 * transitions are not counted; k_steps - burn_in == 2 h with h >= 2 is required; a counted state is the state AFTER the
 * transition; per coordinate, per half and with c = 1 .. h
 *     d = x - mean;   mean = mean + d * recip[c - 1];   M2 = M2 + d * (x - mean)
 * in fp32, every operation rounded on its own, recip[c - 1] = (float)(1.0 / c).
 *
 * BAOAB (sampler = 0; step = h).  The constants hh, c1, c2, sqrt_temp and the recurrence B A O A (g) B of
 * ebm_kinetic_chain_f32, operation for operation: the raw unclamped gradient, the kicks not merged, the start's gradient from
 * one evaluation in front of the loop.  z is the normal field at Philox step offset + 1 + s, element chain * dim + col, or
 * the injected noise[k_steps, n_chains, dim]; draw_v0 != 0 starts from sqrt_temp * z0, z0 at step offset.  A call owns the
 * steps offset .. offset + k_steps: the final x and v equal ebm_kinetic_chain_f32's on the same draws.  n_leapfrog, u,
 * accept_mask and accept_count are ignored.
 *   e_mom   NULL, or float[4][n_chains]: the energy of the post-step position, returned by the one evaluation inside the
 *           step together with the gradient -- that position is the counted state, so no evaluation is added.  With
 *           e_mom == NULL the kernel is another instantiation that carries no group reduction (and writes no e_traj).
 *   v2_mom  NULL, or float[2][n_chains][dim]: the running mean of v^2 per coordinate and half, v the velocity at the END of
 *           the step (behind the closing B):   m = m + (v * v - m) * recip[c - 1],   each operation rounded on its own.  On a
 *           quadratic energy E'' = k its expectation is T (1 - h^2 k / 4): the step-size error read off the run.
 *   v_traj  NULL, or float[n_chains][2 h][dim]: those velocities.  For tests and small runs, as traj and e_traj.
 *
 * GHMC (sampler = 1; step = eps, n_leapfrog = L >= 1).  The constants c1, c2, sqrt_temp, beta and the transition of
 * ebm_ghmc_chain_f32, operation for operation: the O refresh, the uniform drawn in front of the trajectory, n_leapfrog
 * safe-mode leapfrog steps (identity mass, carried energy and force, the pseudo-transition for the start),
 * accepted iff u < min(1, exp(clamp(beta (H0 - H1), +-50))), the velocity flipped on a reject.  z_t at step offset + 1 + 2 t,
 * the uniform at offset + 2 + 2 t, element chain; noise[k_steps, n_chains, dim] / u[k_steps, n_chains] in their place, either
 * without the other; draw_v0 as above.  A call owns the steps offset .. offset + 2 k_steps: the final x, v and the accept mask
 * equal ebm_ghmc_chain_f32's on the same draws.  Counted: the held position and the carried energy; a reject counts the held
 * state again; no evaluation is added.  accept_mask: NULL, or uint8[k_steps][n_chains]; accept_count: NULL, or device
 * uint32[k_steps] the call ADDS to (one atomic per wave and transition).  v2_mom and v_traj must be NULL: the velocity law is
 * exact under the Metropolis correction and carries no information.
 *
 * Outputs.  x and v are updated in place and stored once, mom / e_mom / v2_mom once at the end.  Slots of a lane that hold no
 * column never reach memory.
 *
 * Limits: every analytic energy except EBM_ENERGY_MLP (EBM_EKIND); 1 <= dim <= 256, one vector per lane (EBM_EDIM, in front of
 * any device access); constants only: no clamp, no tables, no mass matrix; 64-bit row indices.  EBM_EINVAL with no buffer
 * touched: a NULL energy, x, v, mom or recip; an unknown sampler; burn_in < 0 or k_steps - burn_in not 2 h with h >= 2; step,
 * gamma or temperature not positive, or NaN (all finite for BAOAB; gamma = +inf, the full refresh, allowed for GHMC);
 * n_leapfrog < 1, a non-NULL v2_mom or a non-NULL v_traj for GHMC.  An empty call (n_chains == 0) returns 0 behind these checks.
 */
EBM_API int ebm_kinetic_moments_f32(const ebm_energy_t* energy, float* x, float* v, int64_t n_chains, int32_t dim,
                                    int32_t sampler, int32_t k_steps, int32_t burn_in, int32_t n_leapfrog, double step,
                                    double gamma, double temperature, int32_t draw_v0, const float* recip, float* mom,
                                    float* e_mom, float* v2_mom, float* traj, float* e_traj, float* v_traj,
                                    uint8_t* accept_mask, uint32_t* accept_count, const float* noise, const float* u,
                                    uint64_t seed, uint64_t offset, void* stream);

/*
 * Per-chain running moments on the MLP energy: the statistics of ebm_kinetic_moments_f32 above -- the same parameter list, the
 * same counted states, recip table, Welford recurrences and layouts of mom, e_mom, v2_mom, traj, e_traj and v_traj -- around the
 * walks of ebm_kinetic_mlp_chain_f32 (sampler = 0, step = h) and ebm_ghmc_mlp_chain_f32 (sampler = 1, step = eps), in ONE launch
 * (an addition to ABI 9: nothing else moved; ebm_kinetic_moments_f32 still refuses the MLP).  One wave walks 32 chains.
 *
 * Walkers.  Those of the two plain MLP entries, operation for operation, with the constants formed by the same host code.
 *   BAOAB: one evaluation site, k_steps + 1 evaluations; evaluation i closes step i - 1 (B) and opens step i (B A O A); the
 *          kicks are never merged; the raw gradient; z_i the normal field at Philox step offset + 1 + i or noise[i].  A call owns
 *          the steps offset .. offset + k_steps.
 *   GHMC:  the O refresh stored back to v; n_leapfrog + 1 evaluations per transition through the safe-mode leapfrog; accepted iff
 *          u < min(1, exp(clamp(beta (H0 - H1), +-50))); a reject flips the stored velocity; z_t at step offset + 1 + 2 t, the
 *          uniform at offset + 2 + 2 t.  A call owns the steps offset .. offset + 2 k_steps.  gamma = +inf is the HMC transition.
 *   draw_v0, noise and u as in the plain entries.  The final x, v and GHMC's accept mask are the plain entries' on the same draws.
 *
 * Counted states.  The first burn_in transitions are not counted; k_steps - burn_in == 2 h with h >= 2; a counted state is the
 * state AFTER the transition; a GHMC reject counts the held state again.  Per coordinate, per half and with c = 1 .. h
 *     d = x - mean;   mean = mean + d * recip[c - 1];   M2 = M2 + d * (x - mean)
 * in fp32, every operation rounded on its own; mom is float[4][n_chains][dim] (mean_a, M2_a, mean_b, M2_b), e_mom NULL or
 * float[4][n_chains].  BAOAB also keeps v2_mom, NULL or float[2][n_chains][dim]:  m = m + (v * v - m) * recip[c - 1]  with v the
 * velocity at the END of the step (behind the closing B), and v_traj, NULL or float[n_chains][2 h][dim], those velocities.
 * traj: NULL, or float[n_chains][2 h][dim], the counted positions; e_traj: NULL, or float[n_chains][2 h], their energies (written
 * with or without e_mom).
 *
 * Energies add no evaluation.  BAOAB: evaluation i >= 1 is made at the position behind step i - 1, the counted state.  GHMC: E'
 * of the proposal on an accept; on a reject the E of the held position that H0 was formed from.  The value counted is the
 * unclamped one.
 *
 * Working storage.  The pairs do not live in registers: mom, e_mom and v2_mom are WORKING STORAGE during the launch -- each
 * counted transition reads a chain's pair from them and writes it back (a lane reads only what it stored itself) -- and defined
 * at return.  At c == 1 the pair starts from zero and the planes are not read: the caller need not initialise them, and whatever
 * they held (a NaN included) never reaches the output.  They must not overlap each other or any other buffer of the call.
 *
 * accept_mask: NULL, or uint8[k_steps][n_chains] (GHMC); accept_count: NULL, or device uint32[k_steps] the call ADDS to (one
 * atomic per wave and transition; GHMC).  Both are ignored for BAOAB, as n_leapfrog and u are.  Columns past dim and rows past
 * n_chains never reach memory; 64-bit row indices.
 *
 * The evaluation is three-way split bf16 (or exact-f32 MFMA) arithmetic with fp32 accumulation: fp32 accuracy, not autograd's
 * rounding.
 *
 * Refusals, all in front of any device access and of the early return for n_chains == 0.  EBM_EINVAL: a NULL energy, x, v, mom
 * or recip; n_chains < 0; an unknown sampler; burn_in < 0 or k_steps - burn_in not 2 h with h >= 2; step, gamma or temperature
 * not positive, or NaN (all finite for BAOAB; gamma = +inf allowed for GHMC); n_leapfrog < 1, a non-NULL v2_mom or a non-NULL
 * v_traj for GHMC.  EBM_EKIND: a kind other than EBM_ENERGY_MLP.  EBM_EDIM: a hidden width (energy->n_comp) other than 64 / 128
 * or dim outside 1 .. 128 (the message names both).  x, v, mom, v2_mom, traj, v_traj and noise must be 16-byte aligned.  No
 * H = 256, no pre-split W1 image (energy->aux is ignored), no tables, no mass matrix.
 */
EBM_API int ebm_kinetic_moments_mlp_f32(const ebm_energy_t* energy, float* x, float* v, int64_t n_chains, int32_t dim,
                                        int32_t sampler, int32_t k_steps, int32_t burn_in, int32_t n_leapfrog, double step,
                                        double gamma, double temperature, int32_t draw_v0, const float* recip, float* mom,
                                        float* e_mom, float* v2_mom, float* traj, float* e_traj, float* v_traj,
                                        uint8_t* accept_mask, uint32_t* accept_count, const float* noise, const float* u,
                                        uint64_t seed, uint64_t offset, void* stream);

/* The accept step with the RNG coordinates in DEVICE memory (rng_state = {seed, step}; the uniforms
 * are drawn at step rng_state[1] + step_delta): the graph-capturable form, see
 * ebm_langevin_step_dev_f32.  No injected-uniform form. */
EBM_API int ebm_hmc_accept_dev_f32(float* x, const float* x_prop, const float* h0, const float* h1,
                           uint8_t* accept_mask, uint32_t* accept_count, int64_t n_chains,
                           int32_t dim, const uint64_t* rng_state, uint64_t step_delta, void* stream);

/*
 * Noise-free descent samplers (reference: torchebm/samplers/gradient_descent.py).
 * torch.sub / torch.add with `alpha` are single-rounding FMAs on the CPU reference, and so are these:
 *   gradient descent (:121-123):   x' = fma(-eta, g(x), x)
 *   Nesterov (:262-266):           la = fma(mu, v, x);  v' = fma(-eta, g(la), fl(v*mu));  x' = x + v'
 * ebm_descent_chain_f32 runs k fused steps for an analytic energy (v starts at zero and is not
 * returned, as in the reference); eta_table = NULL or device float[k]; traj as in the Langevin chain.
 * ebm_descent_step_f32 is one update with an external gradient (v == NULL: plain descent; else v is
 * updated in place); ebm_lookahead_f32 forms the Nesterov look-ahead point.  `out` may alias `x` (the same pointer) in
 * both; `grad` and `v` are distinct from `out` and from each other, and `x` is only read when `out` is another buffer.
 */
EBM_API int ebm_descent_chain_f32(const ebm_energy_t* energy, float* x, int64_t n_chains, int32_t dim,
                                  int32_t k_steps, float eta, const float* eta_table, int32_t nesterov,
                                  float momentum, int32_t thin, float* traj, void* stream);
EBM_API int ebm_descent_step_f32(const float* x, const float* grad, float* v, float* out, int64_t n_elem,
                                 float eta, float momentum, void* stream);
EBM_API int ebm_lookahead_f32(const float* x, const float* v, float* out, int64_t n_elem, float momentum,
                              void* stream);

/*
 * Persistent-CD replay-buffer traffic in one launch each (reference:
 * torchebm/core/base_loss.py:296-315 stratified read, :390-426 FIFO write).
 *   gather:  row_i = (i*stride + r_i) % buffer_size,  r_i uniform in {0..stride-1};  out[i,:] = buffer[row_i,:]
 *            r_i = offsets[i] when offsets != NULL (injected), else floor(o_i * stride / 2^32) with o_i the
 *            raw 32-bit output of the native RNG field at step `offset`, element i.  rows_out (optional)
 *            receives row_i.  stride = buffer_size / batch (>= 1).
 *   scatter: buffer[(write_pos + i) % buffer_size, :] = samples[i, :]   for i < batch <= buffer_size
 */
EBM_API int ebm_pcd_gather_f32(const float* buffer, int64_t buffer_size, int32_t dim, float* out, int64_t batch,
                               int64_t stride, const int64_t* offsets, int64_t* rows_out,
                               uint64_t seed, uint64_t offset, void* stream);
EBM_API int ebm_pcd_scatter_f32(float* buffer, int64_t buffer_size, int32_t dim, const float* samples,
                                int64_t batch, int64_t write_pos, void* stream);

/*
 * ABI 6 -- the three launches of a persistent-CD TRAINING STEP with every per-step coordinate in DEVICE memory, so that the
 * whole step (start points, the k-fused chain, the FIFO write, the caller's loss / backward / optimiser) can be captured in
 * ONE HIP graph and replayed with fresh draws and an advancing write position: what the host would otherwise bake into the
 * kernel arguments at capture time lives in two small device buffers that launches inside the graph read and that a
 * one-element add inside the same graph advances (torchebm_amd/utils/graphed_step.py; reference call sites:
 * torchebm/losses/contrastive_divergence.py:82-155, core/base_loss.py:266-337,390-426).  Same convention as
 * ebm_langevin_step_dev_f32 / ebm_noise_fill_dev_f32: rng_state = {seed, step}; the launch draws at step rng_state[1] + step_delta.
 *   ebm_langevin_chain_dev_f32: ebm_langevin_chain_f32 with native draws (no injected noise, no diagnostics records) at steps
 *       rng_state[1] + step_delta .. + k_steps - 1.  Energies: EBM_ENERGY_MLP (every shape the chain kernel takes); EBM_EKIND
 *       for the others (their kernels take the coordinates by value).  `clamp_on` is the same flag word: unknown bits are
 *       EBM_EINVAL, and EBM_CHAIN_CONTRACTED is accepted and ignored (the MLP kernels never contract).
 *   ebm_pcd_gather_dev_f32: ebm_pcd_gather_f32 with native offsets drawn at step rng_state[1] + step_delta.
 *   ebm_pcd_scatter_dev_f32: ebm_pcd_scatter_f32 with the write position read from *write_pos (device int64, 0 <= *write_pos
 *       < buffer_size; advancing it is the caller's: (pos + batch) % buffer_size).
 */
EBM_API int ebm_langevin_chain_dev_f32(const ebm_energy_t* energy, float* x, int64_t n_chains, int32_t dim,
                                       int32_t k_steps, float eta, float sqrt_eta, float noise_coef,
                                       const float* coef_table, int32_t clamp_on, float cmin, float cmax,
                                       int32_t thin, float* traj, const uint64_t* rng_state, uint64_t step_delta,
                                       void* stream);
EBM_API int ebm_pcd_gather_dev_f32(const float* buffer, int64_t buffer_size, int32_t dim, float* out, int64_t batch,
                                   int64_t stride, int64_t* rows_out, const uint64_t* rng_state, uint64_t step_delta,
                                   void* stream);
EBM_API int ebm_pcd_scatter_dev_f32(float* buffer, int64_t buffer_size, int32_t dim, const float* samples,
                                    int64_t batch, const int64_t* write_pos, void* stream);

/*
 * ABI 7 -- the chain starts of a persistent-CD step in ONE launch: the stratified gather of ebm_pcd_gather_f32 (row i of out = buffer
 * row i stride + U_i, U_i uniform in [0, stride)) AND the reference's exploration noise on a random subset of exactly n_noise rows
 * (core/base_loss.py:316-332: start_points[randperm(batch)[:n_new]] += 0.01 randn; n_noise = max(1, int(batch new_sample_ratio)),
 * noise_scale = 0.01 there).  The subset is { i : pi(i) < n_noise } for a keyed pseudo-random bijection pi of [0, batch) (six-round
 * Feistel network on ceil(log2 batch) bits with cycle walking; round keys from the Philox field): every subset of that size
 * (pseudo-)equally likely, as randperm's prefix is -- no sort, no index list, no torch-side draw, so the step replays from a HIP
 * graph with the same numbers as the eager loop.  Consumes THREE steps of the field: step (offsets, as the gather), step + 1 (round
 * keys: groups 0, 1), step + 2 (the normals, element e of out).  rng_state (optional): {seed, step0} in device memory, `step` is then
 * an offset from step0 and `seed` is ignored (the _dev form of the other entries).  batch < 2^31.  n_noise = 0: the plain gather.
 */
EBM_API int ebm_pcd_start_points_f32(const float* buffer, int64_t buffer_size, int32_t dim, float* out, int64_t batch,
                                     int64_t stride, int64_t n_noise, float noise_scale, uint64_t seed, uint64_t step,
                                     const uint64_t* rng_state, void* stream);

/*
 * ABI 7 -- the contrastive-divergence loss of ONE model call on [data | negatives] (losses/contrastive_divergence.py:128-155):
 *   L = mean(E+) - mean(E-) + reg (mean(E+^2) + mean(E-^2)),   e_both = float[2 n] = E+ | E-;
 * a non-finite L becomes the constant 0.1 and sends no gradient (:150-155).  ebm_cd_loss_f32: one launch -- block partials of the
 * four sums in fp64, added in block order by the last block to finish -- writes loss_out[1] and finite_out[1] (1.0 / 0.0).
 * work: device memory of ebm_cd_loss_work_bytes() bytes, 8-byte aligned, ZEROED once by the caller (the ticket counter in it is left
 * at zero again by every launch, so consecutive calls on one stream share it).  ebm_cd_loss_backward_f32: the per-row seed
 * seed_out[2 n] = dL/dE_i = (+-1 + 2 reg E_i) / n * upstream[0] * finite[0] (upstream: dL_total/dL, a device scalar) -- what
 * ebm_mlp_param_grads_f32 takes as `seed`.  torch's graph of the same arithmetic is some twenty launches of 4 - 5 us.
 */
EBM_API int64_t ebm_cd_loss_work_bytes(void);
EBM_API int ebm_cd_loss_f32(const float* e_both, int64_t n, float reg, void* work, float* loss_out, float* finite_out, void* stream);
EBM_API int ebm_cd_loss_backward_f32(const float* e_both, int64_t n, float reg, const float* upstream, const float* finite,
                                     float* seed_out, void* stream);

/* Energy E(x)[n_chains] and gradient dE/dx[n_chains, dim] of a fused analytic energy
 * (either output may be NULL).  core/base_model.py:143-148,181-210,224-229. */
EBM_API int ebm_energy_grad_f32(const ebm_energy_t* energy, const float* x, int64_t n_chains,
                        int32_t dim, float* energy_out, float* grad_out, void* stream);

/*
 * ABI 6 / 7 -- the forward + backward of a training step through an EBM_ENERGY_MLP network, for the parameter gradients (what autograd
 * does for loss.backward() through the energies of torchebm/losses/contrastive_divergence.py:128-155; the network of
 * examples/20-training/01-mcmc-losses/02-persistent-cd/main.py:21-31).  One launch evaluates the network on x[n, dim], runs the
 * backward through it for a UNIT seed on the matrix cores, everything on-chip, and stores the three activation planes the parameter
 * gradients are made of, in TILES of 32 rows, hidden-major within a tile:
 *   acts = float[n_pad / 32][3][H][32],  n_pad = n rounded up to a multiple of 128 (tile t = rows 32 t .. 32 t + 31, one contiguous
 *   block of 12 H floats -- what one wavefront writes and what one step of ebm_mlp_param_grads_f32 reads; rows n .. n_pad - 1 are
 *   written too, with the values of an all-zero input row: the gradient pass gives them seed 0):
 *   [.][0] h1 = silu(W1 x + b1)   [.][1] a2 = W2 h1 + b2   [.][2] d1 = (W2^T (w3 silu'(a2))) silu'(a1)
 * (ABI 6 stored h1 | seed h2 | seed d2 | seed d1 as [4][H][n_pad]; h2 = silu(a2) and d2 = w3 silu'(a2) are functions of a2 and w3 that the
 * gradient pass recomputes, a quarter of the bytes less).  From these   dW2 = d2 h1^T,  db2 = d2 1,  dW1 = d1 x,  db1 = d1 1,
 * dw3 = h2 1,  db3 = 1   -- each summand weighted with its row's seed -- are small-output products over K = n
 * (ebm_mlp_param_grads_f32 below makes them in one pass).  energy_out (optional): E(x)[n];  grad_out (optional): seed dE/dx [n, dim]
 * (seed[n], NULL = 1, scales grad_out ONLY: the planes are seed-free).  The autograd graph of the same step materialises a1, h1, a2,
 * h2 and their gradients -- some forty passes over [n, H] arrays; this is one.  Hidden width 64 or 128, dim <= 64 (EBM_EDIM
 * otherwise).  With energy_out set it IS the training forward; without a gradient to prepare the forward is ebm_energy_grad_f32 with
 * grad_out = NULL, which runs the forward pass only.
 */
EBM_API int ebm_mlp_backward_acts_f32(const ebm_energy_t* energy, const float* x, int64_t n_chains, int32_t dim,
                                      const float* seed, float* energy_out, float* grad_out, float* acts, void* stream);

/*
 * ABI 7 -- the parameter gradients themselves, from the planes ebm_mlp_backward_acts_f32 stored (acts = float[n_pad / 32][3][H][32]:
 * h1 | a2 | d1) and the rows x[n_rows, dim] they were made from, in ONE pass over the planes:
 *   grads_out = float[H dim + H + H H + H + H + 1], the packed parameter order of EBM_ENERGY_MLP:  dW1 | db1 | dW2 | db2 | dw3 | db3.
 * seed (optional, [n_rows]; NULL = 1): the per-row dL/dE, applied HERE, on load (d1, d2 and h2 are linear in it), so that the ONE
 * ebm_mlp_backward_acts_f32 launch of the forward pass serves the backward pass too.  w3: the last layer's weights [H] (d2 = w3
 * silu'(a2); the packed parameter block + H dim + H + H H + H).  h2 and d2 are recomputed from a2 with the forward kernel's own
 * arithmetic (hardware exp2 / rcp).  The products run on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulation); every
 * workgroup writes one partial record into `work` and a second kernel adds the records in a fixed order: same inputs, same bits,
 * whatever the scheduling.  work: device float[work_floats], work_floats >= ebm_mlp_param_grads_work_f32(hidden, dim, n_rows) (a
 * per-device figure: two records per CU; 0 for an unsupported shape).  Hidden width 64 or 128, dim <= 64 (EBM_EDIM otherwise).
 * Reference: what autograd does for loss.backward() through the nn.Linear weights (torchebm/losses/contrastive_divergence.py:128-155).
 */
EBM_API int64_t ebm_mlp_param_grads_work_f32(int32_t hidden, int32_t dim, int64_t n_rows);
EBM_API int ebm_mlp_param_grads_f32(const float* acts, int64_t n_rows, int32_t hidden, const float* x, int32_t dim, const float* seed,
                                    const float* w3, float* work, int64_t work_floats, float* grads_out, void* stream);

/* Column statistics for the sampler diagnostics (samplers/langevin_dynamics.py:173-185):
 * mean[dim], biased var[dim] clamped to [1e-10, 1e10].  `work` = device double[2*dim + 1], zeroed once by
 * the caller: the kernel's last block finishes the statistics and leaves it zeroed again, so consecutive
 * calls on one stream share it without a memset.  Sums are shifted by row 0 and kept in double; for dim a power of two in
 * [4, 1024] (and n_chains * dim >= 1024) the shifted values are formed and summed four rows at a time in fp32 first, so the
 * accuracy of that path is relative to the spread about row 0 -- |d var| <= U var + 14 U mean((x - x[0])^2), U = 2^-24 -- not
 * to the variance: a first row far from all the others costs it accuracy (tests/chain_stats_cases.py derives the bounds). */
EBM_API int ebm_chain_stats_f32(const float* x, int64_t n_chains, int32_t dim, float* mean_out,
                        float* var_out, double* work, void* stream);

/* Fill `out[n_elem]` with the native RNG field at step `offset` (tests / verification /
 * BaseSampler._init_state-style draws): normals, uniforms in [0,1), or raw u32 bits. */
EBM_API int ebm_noise_fill_f32(float* out, int64_t n_elem, int32_t kind, uint64_t seed,
                       uint64_t offset, void* stream);

/* The same field with {seed, step} read from DEVICE memory, at step rng_state[1] + step_delta (the
 * momentum draw of a HMC transition captured in a HIP graph, samplers/hmc.py:92-134). */
EBM_API int ebm_noise_fill_dev_f32(float* out, int64_t n_elem, int32_t kind, const uint64_t* rng_state,
                           uint64_t step_delta, void* stream);

/*
 * In-kernel sampler diagnostics (SURVEY.md section 8b `diag_partials`, section 5 "kernels emit per-block partial sums").
 * At every kept step each workgroup of a chain launch stores ONE record of its chains' per-column partials
 * (sum, M2 about the block mean), its energy sum and its accept count; ebm_diag_finish_f32 merges the records of
 * all kept steps into the reference's diagnostics tensors.  return_diagnostics=True is therefore one chain launch
 * plus one small merge launch, with no extra pass over the state.  (The matrix-layout MLP kernels store one record per
 * WAVEFRONT of 32 chains -- the state lives in the MFMA accumulator layout, a column statistic is a sum over 32 lanes, no
 * LDS tile -- and write a Langevin record's energy share one evaluation late, when the energy of the kept state exists;
 * a kept last step costs one forward pass more.  Since ABI version 3.)
 *
 * ebm_diag_layout: the record geometry the chain entry WOULD use for this energy / shape --
 *   sampler: EBM_DIAG_LANGEVIN / EBM_DIAG_LANGEVIN_HEUN / EBM_DIAG_HMC;  injected_noise / with_traj: whether the
 *   chain call will pass a noise / trajectory pointer (they select the kernel family);
 *   outputs: n_blocks (records per kept step), slots S and block_elems E.  The caller allocates
 *   diag_partials = float[n_kept][n_blocks][2*S + 8] and work = double[n_kept][3*dim + 3] (zeroed once; the merge
 *   leaves it zeroed; 3*max(S, dim) + 3 doubles per kept step when S > dim, below).  (Dense Gaussians above 128 dims: records from the
 *   streamed-Ps kernels, csrc/gauss_big.hip, for multiples of 4 up to 512.)  S > dim means PACKED rows: a dense
 *   Gaussian whose width the matrix-layout kernel does not take as is (below 20, or not a multiple of 4) runs S / dim
 *   consecutive chains as one row of width S (block-diagonal precision; same element order, same random field), and
 *   the records are those of n_chains * dim / S rows: call ebm_diag_finish_f32 with (n_chains * dim / S, S) and fold
 *   the S columns onto the dim coordinates -- mean = average of the S / dim column means of a coordinate, var = average
 *   of their variances + the (biased) variance of those column means, energy divided by S / dim
 *   (torchebm_amd/samplers/langevin.py, _fused_with_records).
 *   block_elems < 0 (since ABI version 5) means records of INTERLEAVED ALIGNMENT CLASSES: the shifted-row kernels (dense
 *   Gaussians and mixtures at widths that are not a multiple of 4, 17 .. 254) give a workgroup the chains of ONE alignment
 *   class -- K = 4 / gcd(dim, 4) classes (4 for an odd width, 2 for width = 2 mod 4) -- so record b = (group b / K, class b % K)
 *   holds the 32 chains 32 K g + K m + s, m = 0 .. 31, of group g = b / K and class s = b % K; block_elems = -32 * dim,
 *   slots = dim, and n_blocks = ceil(n_chains / (32 K)) * K.  Treat the value as opaque: allocate diag_partials with the
 *   n_blocks and slots returned and hand block_elems to ebm_diag_finish_f32 unchanged (it accepts the negative form); a caller
 *   that computes with block_elems itself must take |block_elems| / dim = 32 chains per record and the interleaving above.
 *   Returns EBM_EDIM / EBM_EKIND when the configuration has no in-kernel form (then take the
 *   statistics from the state with ebm_chain_stats_f32 / ebm_energy_grad_f32 between launches).
 * ebm_diag_finish_f32: mean_out / var_out = float[n_kept][dim] (biased variance clamped to [1e-10, 1e10], zero for a
 *   single chain), energy_out = float[n_kept] (mean per-chain energy), accept_out = NULL or float[n_kept]
 *   (accepted fraction of the kept transition).  fp64 merge by the pairwise-variance identity.
 */
enum { EBM_DIAG_LANGEVIN = 0, EBM_DIAG_LANGEVIN_HEUN = 1, EBM_DIAG_HMC = 2 };
EBM_API int ebm_diag_layout(const ebm_energy_t* energy, int32_t sampler, int64_t n_chains, int32_t dim,
                            int32_t injected_noise, int32_t with_traj, int64_t* n_blocks, int32_t* slots,
                            int32_t* block_elems);
EBM_API int ebm_diag_finish_f32(const float* diag_partials, int32_t n_kept, int64_t n_blocks, int32_t slots,
                                int32_t block_elems, int64_t n_chains, int32_t dim, float* mean_out, float* var_out,
                                float* energy_out, float* accept_out, double* work, void* stream);

/* Measurement aid (bench.py, no counterpart in the reference): `blocks` x 256 lanes each issue
 * 8 * iters independent v_fma_f32.  blocks * 4 * 8 * iters wave-instructions / elapsed time = the plain-VALU
 * issue rate of this chip at its current clock, against which the VALU-bound chain kernels are priced.
 * `out` = float[blocks * 256] (keeps the arithmetic alive). */
EBM_API int ebm_probe_valu_f32(float* out, int32_t blocks, int32_t iters, void* stream);

/* The same stream shape with the instruction classes the in-kernel RNG is made of, so that bench.py can price the
 * Langevin loop from costs measured in the run instead of constants: per lane and iteration,
 *   kind 0: 8 v_fma_f32 (= ebm_probe_valu_f32)          kind 1: 8 x (v_mad_u64_u32 + v_xor_b32)
 *   kind 2: 8 x (v_log_f32 + v_add_f32)                 kind 3: 8 v_pk_fma_f32 (16 fused multiply-adds; SGPR-pair multiplicand)
 *   kind 4: 8 v_bitop3_b32                              kind 5: 8 v_pk_fma_f32, every operand a VGPR pair
 *   kind 6: 8 v_pk_mul_f32
 *   kind 7: the lean Langevin loop's static mix per float4 group and step -- 18 v_mad_u64_u32, 20 v_bitop3_b32, 8 transcendentals,
 *           20 packed-f32 (14 v_pk_mul_f32 + 6 v_pk_add_f32), 10 plain (76 instructions per iteration; `iters` even), dependency-free: the ceiling of a kernel made of that mix
 * independent across the eight slots (`iters` a multiple of 4 for kinds 3 / 5 / 6).  Since ABI version 3. */
EBM_API int ebm_probe_issue_f32(float* out, int32_t blocks, int32_t iters, int32_t kind, void* stream);

/* The pre-split first-layer image of an EBM_ENERGY_MLP network (see the enum: ebm_energy_t.aux).  Both weight matrices as
 * bf16 triples are 192 KB at H = 128 and dim > 64 -- more than a CU's LDS -- so the W1 triple is laid out once in global
 * memory (the caller's buffer, 16-byte aligned, ebm_mlp_w1_image_bytes() long; 0 = this shape has no image) in the order the
 * chain kernel streams it through LDS.  Rebuild it whenever the parameters change (one small kernel; stream-ordered like every
 * entry).  No counterpart in the reference: there the network is nn.Linear modules evaluated by autograd every step
 * (samplers/langevin_dynamics.py:168-172).  Since ABI version 4. */
/* The same for an EBM_ENERGY_GAUSSIAN precision matrix at dims 132 .. 512 (multiples of 4): the three bf16 pieces of P
 * (hi + mid + lo = the fp32 value) in the order the stages of the tiled Langevin kernel consume them, 1.5 x the size of P --
 * and, since ABI version 5, at the widths 158 .. 254 that are not a multiple of 4: one image per alignment class of the
 * shifted rows (K = 4 / gcd(dim, 4) of them, each laid out for the row shifted by that class's offset), K x the size.
 * `prec` is the SYMMETRIC matrix handed over as dev1.  0 bytes = this width has no image.  Since ABI version 4. */
EBM_API size_t ebm_gauss_prec_image_bytes(int32_t dim);
EBM_API int ebm_gauss_prec_image_f32(const float* prec, int32_t dim, void* image, void* stream);

/* The active-column hint of EBM_ENERGY_GMM (its `aux`), computed on the device in ONE small launch (since ABI version 5):
 * out[0] = sum_v 2^v * [ the component means differ somewhere in columns 4v..4v+3 ],  means [n_comp, dim], dim % 4 == 0,
 * dim <= 32.  Replaces the seven tensor ops the Python model spent on it at every sample() call (45 us of launches in
 * front of a 0.1 - 1 ms kernel).  `!=` as IEEE: a NaN mean differs from everything. */
EBM_API int ebm_gmm_active_columns_i32(const float* means, int32_t n_comp, int32_t dim, int32_t* out, void* stream);

EBM_API size_t ebm_mlp_w1_image_bytes(int32_t hidden, int32_t dim);
EBM_API int ebm_mlp_w1_image_f32(const float* params, int32_t hidden, int32_t dim, void* image, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EBM_HIP_H */
