"""One evaluation of every fused chain route against float64 (tests/chain_cases.py ROUTES).

The matrix-core kernels contract on the bf16 pipe with operands split three ways (gauss_bf16x3.h, gmm_bf16x3.h,
mfma_hmc_body.h, gauss_stream_e.h); the design says that is as accurate as fp32.  The chain-level tests compare with the fp32
oracle at 5e-4 and would not see a kernel that dropped one term of the split (about 1.5e-5 relative per product).  Here:
  * Langevin / Heun: one noise-free step, k = 1, noise_coef = 0 (the _fast kernels) and again with an injected all-zero
    noise field and noise_coef != 0 (the kernels that read a noise field), against x0 - eta grad E(x0) in float64 of the
    fp32 parameters the kernel was handed;
  * HMC: one transition of one leapfrog step with injected momenta and u = 0 (always accepted): the returned state against
    x0 + eps (p sqrt(m) - eps/2 grad E(x0)) / m in float64, with the force term dominating the natural scale;
  * HMC accept decisions with u injected just below / above the float64 acceptance probability, at a relative margin of
    C_H U (N(H0) + N(H1)) + C_EXP 2^-23: a kernel whose energy is only bf16-accurate decides some of them wrongly.
The bars and their constants are set on the CPU (tests/test_fp64_bars.py): an fp32 evaluation meets them, two-term bf16
operands fail them."""

import pytest
import torch

import chain_cases as cc
from helpers import yardstick

pytestmark = pytest.mark.gpu

LANGEVIN = [c for c in cc.ROUTES if c.sampler != "hmc"]
HMC = [c for c in cc.ROUTES if c.sampler == "hmc"]


def langevin_eta(case):
    return 0.25 if case.energy == "gauss" else 0.5


def check_langevin(case, x0, fp, got):
    eta = langevin_eta(case)
    want, natural = cc.langevin_ref(case, x0, fp, eta)
    err = (got.double() - want).abs()
    if case.energy == "gauss":
        rel = (err / natural)
        worst = rel.max().item()
        i, j = divmod(int(rel.argmax()), case.dim)
        assert worst < cc.k_step(case.dim) * cc.U, (case.id, worst / cc.U, "chain", i, "coordinate", j)
        return worst / cc.U
    # the mixtures form squared distances as |x|^2 - 2 x.mu + |mu|^2 (csrc/gmm_bf16x3.h, the comment of
    # test_mixture_matrix_path_gradient_is_fp32_accurate in tests/test_edge_cases_gpu.py): bars on that expansion's scale,
    # and no further from float64 than torch's own fp32 step as a population
    # (not at dim 2, the pair kernel: there is no contraction, a row's error is one or two ulps of the result, and the ratio
    #  of two such medians is quantisation -- 1.1e-7 against torch's 5.4e-8 at 0.6 U of the bar below)
    if case.dim > 2:
        yardstick(got, cc.langevin_ref32(case, x0, fp, eta), want, k_med=2.0, k_max=16.0, what=case.id)
    worst = (err.amax(dim=1) / natural).max().item()
    assert worst < cc.K_GMM * cc.U, (case.id, worst / cc.U, int((err.amax(dim=1) / natural).argmax()))
    return worst / cc.U


@pytest.mark.parametrize("noise_field", [False, True], ids=["fast", "noise"])
@pytest.mark.parametrize("case", LANGEVIN, ids=lambda c: c.id)
def test_langevin_step_is_fp32_accurate(cuda_device, case, noise_field):
    _, spec, fp = cc.device_model(case, cuda_device)
    x0 = cc.langevin_x0(case, fp)
    got = cc.run_langevin(case, spec, x0, langevin_eta(case), noise_field, cuda_device).x
    check_langevin(case, x0, fp, got)


def hmc_setup(case, cuda_device):
    _, spec, fp = cc.device_model(case, cuda_device)
    x0, p, mass = cc.hmc_inputs(case, fp)
    return spec, fp, x0, p, mass


@pytest.mark.parametrize("case", HMC, ids=lambda c: c.id)
def test_hmc_leapfrog_step_is_fp32_accurate(cuda_device, case):
    spec, fp, x0, p, mass = hmc_setup(case, cuda_device)
    eps = cc.hmc_eps(case, x0, p, mass, fp, target=1.0 if case.energy == "gauss" else cc.GMM_FORCE_TARGET)
    want, natural, gmax = cc.hmc_ref(case, x0, p, mass, fp, eps)
    assert gmax < 1e5  # the force clamp at 1e6 is not reached
    run = cc.run_hmc(case, spec, x0, p, torch.zeros(case.n), mass, eps, cuda_device)
    got, mask = run.x, run.mask[0]
    assert bool((mask == 1).all()), "u = 0 accepts every proposal"
    err = (got.double() - want).abs()
    if case.energy == "gauss":
        rel = err / natural
        i, j = divmod(int(rel.argmax()), case.dim)
        assert rel.max().item() < cc.k_step(case.dim) * cc.U, (case.id, rel.max().item() / cc.U, "chain", i, "coordinate", j)
        return
    yardstick(got, cc.hmc_ref32(case, x0, p, mass, fp, eps), want, k_med=2.0, k_max=16.0, what=case.id)
    rel = err.amax(dim=1) / natural
    assert rel.max().item() < cc.K_GMM * cc.U, (case.id, rel.max().item() / cc.U, int(rel.argmax()))


@pytest.mark.parametrize("case", HMC, ids=lambda c: c.id)
def test_hmc_accept_decision_resolves_the_fp64_energy(cuda_device, case):
    spec, fp, x0, p, mass = hmc_setup(case, cuda_device)
    x0 = cc.hmc_accept_x0(case, x0, fp)
    eps = cc.hmc_accept_eps(case, x0, p, mass, fp)
    h0, h1, n0, n1 = cc.hmc_hamiltonians64(case, x0, p, mass, fp, eps)
    keep, u, below = cc.accept_draws(h0, h1, n0, n1)
    assert keep.sum().item() >= case.n // 4, keep.sum().item()
    assert (keep & below).any() and (keep & ~below).any()
    mask = cc.run_hmc(case, spec, x0, p, u, mass, eps, cuda_device).mask[0]
    wrong = keep & (mask.bool() != below)
    assert not wrong.any(), (case.id, wrong.nonzero().flatten()[:8].tolist(), int(wrong.sum()))
