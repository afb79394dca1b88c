"""The bars of tests/test_fp64_one_step_gpu.py, on the CPU: the fp32 oracle's own evaluation (oracle.Gaussian /
oracle.GaussianMixture in fp32) meets each of them, and the same evaluation with a contraction whose operands are rounded
to a TWO-term bf16 split (hi = bf16(a), lo = bf16(a - hi), the third piece dropped) fails each of them.  These set the
constants of tests/chain_cases.py (k_step, K_GMM, GMM_FORCE_TARGET, C_H, C_EXP) -- none is tuned against a GPU."""

import pytest
import torch

import chain_cases as cc
from helpers import yardstick


def split2(a):
    """a as the sum of its two leading bf16 pieces, in float64 (products of such pieces are exact there)."""
    a = a.float()
    hi = a.bfloat16().float()
    lo = (a - hi).bfloat16().float()
    return hi.double() + lo.double()


def gauss_grad_split2(x, fp):
    mean, ps = fp
    return split2(x - mean) @ split2(ps).t()


def gmm_grad_split2(x, fp):
    """the kernels' form: |x|^2 - 2 x.mu + |mu|^2 with x.mu on split operands, then the weighted means the same way."""
    means, sigma, logw = fp
    x = x.float()
    sq = (x.double().square().sum(1, keepdim=True) - 2 * (split2(x) @ split2(means).t()) +
          means.double().square().sum(1)[None]).float().double()
    w = torch.softmax(logw.double()[None] - sq / (2 * sigma ** 2), dim=1)
    return (x.double() - split2(w) @ split2(means)) / sigma ** 2


def grad_split2(case, x, fp):
    return gauss_grad_split2(x, fp) if case.energy == "gauss" else gmm_grad_split2(x, fp)


def _case(sampler, energy, dim, K=0, mass="none", n=300):
    return cc.Case(sampler, energy, dim, K=K, mass=mass, n=n)


def langevin_bar_holds(case, x0, fp, got):
    eta = 0.25 if case.energy == "gauss" else 0.5
    want, natural = cc.langevin_ref(case, x0, fp, eta)
    err = (got.double() - want).abs()
    if case.energy == "gauss":
        return (err / natural).max().item() < cc.k_step(case.dim) * cc.U
    try:
        yardstick(got, cc.langevin_ref32(case, x0, fp, eta), want, k_med=2.0, k_max=16.0)
    except AssertionError:
        return False
    return (err.amax(dim=1) / natural).max().item() < cc.K_GMM * cc.U


LANGEVIN_SAMPLE = [_case("langevin", "gauss", d, n=n) for d, n in ((10, 320), (20, 300), (64, 300), (157, 300), (254, 300), (512, 200))] + \
                  [_case("langevin", "gmm", d, K) for d, K in ((20, 8), (64, 16), (128, 32), (200, 12), (255, 16))]


@pytest.mark.parametrize("case", LANGEVIN_SAMPLE, ids=lambda c: c.id)
def test_langevin_bars(case):
    fp = cc.cpu_params(case)
    x0 = cc.langevin_x0(case, fp)
    eta = 0.25 if case.energy == "gauss" else 0.5
    assert langevin_bar_holds(case, x0, fp, cc.langevin_ref32(case, x0, fp, eta)), "the fp32 oracle misses the bar"
    two = (x0.double() - eta * grad_split2(case, x0, fp)).float()
    assert not langevin_bar_holds(case, x0, fp, two), "a two-term bf16 contraction passes the bar"


def test_heun_bar_is_met_by_the_oracle():
    case = _case("heun", "gauss", 64)
    fp = cc.cpu_params(case)
    x0 = cc.langevin_x0(case, fp)
    assert langevin_bar_holds(case, x0, fp, cc.langevin_ref32(case, x0, fp, 0.25))


# (a thousand Gaussian chains: above 200 dims two-term energies misdecide only two to eight of the ~570 kept ones)
HMC_SAMPLE = [_case("hmc", "gauss", d, mass=m, n=1000) for d, m in ((20, "none"), (64, "diag"), (160, "scalar"), (200, "none"), (255, "none"))] + \
             [_case("hmc", "gmm", d, K, mass=m) for d, K, m in ((20, 8, "none"), (96, 16, "diag"), (228, 16, "none"))]


def hmc_bar_holds(case, x0, p, mass, fp, eps, got):
    want, natural, _ = cc.hmc_ref(case, x0, p, mass, fp, eps)
    err = (got.double() - want).abs()
    if case.energy == "gauss":
        return (err / natural).max().item() < cc.k_step(case.dim) * cc.U
    try:
        yardstick(got, cc.hmc_ref32(case, x0, p, mass, fp, eps), want, k_med=2.0, k_max=16.0)
    except AssertionError:
        return False
    return (err.amax(dim=1) / natural).max().item() < cc.K_GMM * cc.U


@pytest.mark.parametrize("case", HMC_SAMPLE, ids=lambda c: c.id)
def test_hmc_position_bars(case):
    fp = cc.cpu_params(case)
    x0, p, mass = cc.hmc_inputs(case, fp)
    eps = cc.hmc_eps(case, x0, p, mass, fp, target=1.0 if case.energy == "gauss" else cc.GMM_FORCE_TARGET)
    assert hmc_bar_holds(case, x0, p, mass, fp, eps, cc.hmc_ref32(case, x0, p, mass, fp, eps)), "the fp32 oracle misses the bar"
    m = torch.ones(case.dim, dtype=torch.float64) if mass is None else (
        torch.full((case.dim,), mass, dtype=torch.float64) if isinstance(mass, float) else mass.double())
    ps = p.double() * m.sqrt()
    two = (x0.double() + eps * (ps - 0.5 * eps * grad_split2(case, x0, fp)) / m).float()
    assert not hmc_bar_holds(case, x0, p, mass, fp, eps, two), "a two-term bf16 force passes the bar"


def energy_split2(case, x, fp):
    if case.energy == "gauss":
        mean, ps = fp
        d = (x - mean).double()
        return 0.5 * (split2(d.float()) * (split2(d.float()) @ split2(ps).t())).sum(dim=1)
    means, sigma, logw = fp
    x = x.float()
    sq = (x.double().square().sum(1, keepdim=True) - 2 * (split2(x) @ split2(means).t()) + means.double().square().sum(1)[None])
    return -torch.logsumexp(logw.double()[None] - sq.float().double() / (2 * sigma ** 2), dim=1)


@pytest.mark.parametrize("case", HMC_SAMPLE, ids=lambda c: c.id)
def test_hmc_accept_bars(case):
    """the margin delta: the fp32 oracle's H0, H1 decide every kept chain as float64 does; H from two-term bf16 contractions
    (on the same fp32 leapfrog state) decide some of them wrongly."""
    fp = cc.cpu_params(case)
    x0, p, mass = cc.hmc_inputs(case, fp)
    x0 = cc.hmc_accept_x0(case, x0, fp)
    eps = cc.hmc_accept_eps(case, x0, p, mass, fp)
    h0, h1, n0, n1 = cc.hmc_hamiltonians64(case, x0, p, mass, fp, eps)
    keep, u, below = cc.accept_draws(h0, h1, n0, n1)
    assert keep.sum().item() >= case.n // 4

    def decisions(e0, e1):
        a = torch.exp((e0 - e1).clamp(-50, 50)).clamp(max=1.0)
        return u.double() < a

    H0, H1 = cc.hmc_hamiltonians32(case, x0, p, mass, fp, eps)
    assert not (keep & (decisions(H0.double(), H1.double()) != below)).any(), "the fp32 oracle decides a kept chain wrongly"
    en = cc._oracle32(case, fp)
    pm = p.clone() if mass is None else p * (mass ** 0.5 if isinstance(mass, float) else mass.sqrt())
    x1, p1 = cc.oracle.hmc.leapfrog(en, x0, pm, eps, 1, mass, safe=True)
    k0, k1 = cc.oracle.hmc.kinetic(pm, mass).double(), cc.oracle.hmc.kinetic(p1, mass).double()
    b0, b1 = energy_split2(case, x0, fp) + k0, energy_split2(case, x1, fp) + k1
    assert (keep & (decisions(b0, b1) != below)).any(), "two-term bf16 energies decide every kept chain as float64 does"
