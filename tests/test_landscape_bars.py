"""The bars of tests/landscape_cases.py hold what they claim, on the CPU: the package's own fp32 path (forward, autograd
gradient -- the reference's lines) meets them on the tests' own seeded inputs, and a deliberately degraded evaluation (the
float64 gradient of inputs rounded to 16 significant bits) fails them in every case.  Also the accept-decision setup of
tests/test_landscape_gpu.py: at least 40 % of the chains of every case are kept and torch's fp32 decides every one of them
as float64 does."""

import pytest
import torch

import landscape_cases as lc
import oracle
from chain_cases import accept_draws


@pytest.mark.parametrize("name", lc.ENERGIES)
def test_cpu_fp32_meets_the_bars_and_a_16_bit_operand_does_not(name):
    m = lc.model(name)
    worst_e = worst_g = 0.0
    degraded_best = float("inf")
    for dim in lc.WIDTHS:
        for scale in lc.SCALES:
            x = lc.inputs(name, dim, scale)
            e, g = lc.cpu32(m, x)
            ee, eg = lc.errors(name, m, x, e, g)
            worst_e, worst_g = max(worst_e, ee), max(worst_g, eg)
            ng, _ = lc.natural(name, m, x)
            d = ((lc.degraded_grad(name, m, x) - lc.grad64(name, m, x)).abs() / (lc.U * ng)).max().item()
            degraded_best = min(degraded_best, d)
            assert d > lc.BAR[name]["grad"], (name, dim, scale, d)
    print(name, "cpu fp32 worst: energy %.3f gradient %.3f; degraded gradient, best case %.1f" % (worst_e, worst_g, degraded_best))
    assert worst_e <= lc.BAR[name]["energy"] and worst_g <= lc.BAR[name]["grad"], (worst_e, worst_g)
    # the constants in the helper are what this loop measures (another host's torch may add a row in another order)
    assert worst_e <= 1.5 * lc.CPU_WORST[name]["energy"] and worst_g <= 1.5 * lc.CPU_WORST[name]["grad"]
    assert degraded_best > 4.0 * lc.BAR[name]["grad"]


def test_natural_scales_bound_the_quantities():
    for name in lc.ENERGIES:
        m = lc.model(name)
        x = lc.inputs(name, 33, 5.0)
        ng, ne = lc.natural(name, m, x)
        assert (lc.grad64(name, m, x).abs() <= ng * (1 + 1e-12)).all()
        assert (lc.energy64(name, m, x).abs() <= ne * (1 + 1e-12)).all()


def test_ackley_gradient_at_the_origin_is_nan_in_the_reference_path():
    g = lc.model("ackley").gradient(torch.zeros(2, 5))
    assert torch.isnan(g).all()


@pytest.mark.parametrize("name", lc.ENERGIES)
def test_accept_setup_keeps_enough_chains_and_fp32_decides_them(name):
    a32 = lc.Adapter(name)
    for dim in (2, 17, 64, 260):
        x, p, eps, (h0, h1, n0, n1) = lc.accept_batch(name, dim)
        keep, u, below = accept_draws(h0, h1, n0, n1)
        xe, pe = oracle.hmc.leapfrog(a32, x, p, eps, 1, None, safe=True)
        H0 = a32.energy(x) + 0.5 * p.square().sum(1)
        H1 = a32.energy(xe) + 0.5 * pe.square().sum(1)
        acc = u < torch.exp((H0 - H1).clamp(-50.0, 50.0)).clamp(max=1.0)
        share = keep.float().mean().item()
        print(name, dim, "eps", eps, "kept share %.3f" % share)
        assert share >= 0.40, (name, dim, share)
        assert bool((acc[keep] == below[keep]).all()), (name, dim)


@pytest.mark.parametrize("name", ["ackley", "rosenbrock"])
def test_safe_mode_inputs_are_not_amplified(name):
    """The inputs of the GPU safe-mode tests: the oracle's own fp32 and float64 runs agree far inside the 5e-4 (tame rows)
    and 1e-3 (wild rows) the GPU test asks of the kernel (T L = 12 at eps = 0.01), so those numbers measure the kernel and
    not the dynamics.  Ackley's wild rows start at the origin, where float64 has the same NaN gradient and runs the same
    scrubs: they are compared too.  Rosenbrock's wild rows overflow in fp32 and not in float64 -- float64 is no referee
    for them; the oracle's fp32 run rejects every proposal of theirs, so their values are the start's, exactly."""
    for dim in (4, 20, 260):
        x0 = lc.inputs(name, dim, 0.5, n=200, salt=12 if name == "ackley" else 13)
        wild = torch.zeros(200, dtype=torch.bool)
        if name == "ackley":
            wild[::3] = True
            x0[wild] = 0.0
        g = torch.Generator().manual_seed(77)
        T, L, eps = 3, 4, 0.01
        p, u = torch.randn(T, 200, dim, generator=g), torch.rand(T, 200, generator=g)
        r32 = oracle.hmc_chain(lc.Adapter(name), x0, p, u, [eps] * T, L)
        r64 = oracle.hmc_chain(lc.Adapter(name, f64=True), x0.double(), p.double(), u.double(), [eps] * T, L, forced_accept=r32["accepted"])
        assert torch.equal(torch.isfinite(r32["x"]), torch.isfinite(r64["x"])) and torch.isfinite(r32["x"]).all()
        rel = (r32["x"].double() - r64["x"]).abs() / r64["x"].abs().clamp(min=1.0)
        assert rel[~wild].max().item() < 5e-5, (name, dim, rel[~wild].max().item())
        if wild.any():
            assert rel[wild].max().item() < 1e-4, (name, dim, rel[wild].max().item())
