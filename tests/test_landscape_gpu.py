"""The fused Rosenbrock / Ackley / Rastrigin energies on the GPU: routes, numerical bars against float64, structure of the
chain calls, HMC safe mode and accept decisions, records, and the law of the samples.  References and bars:
tests/landscape_cases.py (the package's own CPU fp32 path is the yardstick, float64 the referee)."""

import math

import pytest
import torch

import landscape_cases as lc
import oracle
import torchebm_amd as ta
from chain_cases import Case, accept_draws, diag_finish, merge_records64, run_hmc, run_langevin
from helpers import hip_calls, launched_kernels, yardstick
from torchebm_amd import _lib
from torchebm_amd.samplers.langevin import em_coefficients

pytestmark = pytest.mark.gpu

P_MIN = 1e-3  # tests/test_ks_gpu.py


def _spec(name, dev):
    return lc.model(name, device=dev).fused_spec()


def _energy_grad(name, x, dev):
    n, dim = x.shape
    xd = x.to(dev).contiguous()
    e, g = torch.full((n,), 7.0, device=dev), torch.full((n, dim), 7.0, device=dev)
    _lib.call("ebm_energy_grad_f32", _spec(name, dev).to_c(), xd.data_ptr(), n, dim, e.data_ptr(), g.data_ptr(), _lib.stream_handle(dev))
    torch.cuda.synchronize()
    return e.cpu(), g.cpu()


# ----------------------------------------------------------------------------------------------------------------
# routes
# ----------------------------------------------------------------------------------------------------------------
def _step_counters():
    return {k: v for k, v in _lib.call_counts.items() if k.startswith(("ebm_langevin_step", "ebm_leapfrog", "ebm_hmc_accept"))}


@pytest.mark.parametrize("name", lc.ENERGIES)
def test_sample_is_one_fused_launch(cuda_device, name):
    m = lc.model(name, device=cuda_device)
    x0 = lc.inputs(name, 20, 0.5, n=500).to(cuda_device)
    before, steps = hip_calls("ebm_langevin_chain_f32"), _step_counters()
    with launched_kernels() as k:
        out = ta.LangevinDynamics(m, step_size=1e-4, device=cuda_device).sample(x=x0.clone(), n_steps=7)
    assert hip_calls("ebm_langevin_chain_f32") == before + 1 and _step_counters() == steps
    assert any("langevin_chain_rows_kernel" in s for s in k.names), k.names
    assert out.shape == x0.shape and torch.isfinite(out).all()

    before, steps = hip_calls("ebm_hmc_chain_f32"), _step_counters()
    with launched_kernels() as k:
        out = ta.HamiltonianMonteCarlo(m, step_size=1e-3, n_leapfrog_steps=3, device=cuda_device).sample(x=x0.clone(), n_steps=4)
    assert hip_calls("ebm_hmc_chain_f32") == before + 1 and _step_counters() == steps
    assert any("hmc_chain_kernel" in s for s in k.names), k.names
    assert out.shape == x0.shape and torch.isfinite(out).all()


# ----------------------------------------------------------------------------------------------------------------
# energy and gradient against float64, every lane geometry
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lc.ENERGIES)
def test_energy_and_gradient_meet_the_bars(cuda_device, name):
    m = lc.model(name)
    worst_e = worst_g = 0.0
    report = []
    for dim in lc.WIDTHS:
        for scale in lc.SCALES:
            x = lc.inputs(name, dim, scale)
            e, g = _energy_grad(name, x, cuda_device)
            ee, eg = lc.errors(name, m, x, e, g)
            report.append((dim, scale, round(ee, 2), round(eg, 2)))
            worst_e, worst_g = max(worst_e, ee), max(worst_g, eg)
    print(name, "worst energy %.3f (bar %.3f)  worst gradient %.3f (bar %.3f)" % (worst_e, lc.BAR[name]["energy"], worst_g, lc.BAR[name]["grad"]))
    print(report)
    bad = [r for r in report if not (r[2] <= lc.BAR[name]["energy"] and r[3] <= lc.BAR[name]["grad"])]
    assert not bad, bad


def test_ackley_other_frequency_takes_the_product_form(cuda_device):
    """c != 2 pi: sin / cos of the fp32 product c x.  Its argument rounding is part of the natural scale (|c x| U)."""
    m = ta.core.AckleyModel(a=20.0, b=0.2, c=3.0)
    for dim in (3, 33, 260):
        x = lc.inputs("ackley", dim, 5.0, salt=3)
        n = x.shape[0]
        xd = x.to(cuda_device)
        e, g = torch.empty(n, device=cuda_device), torch.empty(n, dim, device=cuda_device)
        _lib.call("ebm_energy_grad_f32", m.fused_spec().to_c(), xd.data_ptr(), n, dim, e.data_ptr(), g.data_ptr(), _lib.stream_handle(cuda_device))
        ee, eg = lc.errors("ackley", m, x, e.cpu(), g.cpu())
        e32, g32 = lc.cpu32(m, x)
        ce, cg = lc.errors("ackley", m, x, e32, g32)
        print(dim, "kernel", ee, eg, "cpu fp32", ce, cg)
        assert ee <= lc.BAR["ackley"]["energy"] and eg <= lc.BAR["ackley"]["grad"]


def test_ackley_gradient_at_the_origin_is_nan_as_autograd_gives_it(cuda_device):
    for dim in (2, 5, 64, 257, 1024):
        x = lc.inputs("ackley", dim, 1.0, n=6)
        x[1] = 0.0
        x[4] = 0.0
        e, g = _energy_grad("ackley", x, cuda_device)
        ref = lc.model("ackley").gradient(x)
        assert torch.isnan(ref[1]).all() and torch.isnan(ref[4]).all()
        assert torch.equal(torch.isnan(g), torch.isnan(ref)), dim
        assert torch.isfinite(e).all() and e[1].abs().item() < 1e-5


# ----------------------------------------------------------------------------------------------------------------
# one step of every chain kernel: no further from float64 than the CPU fp32 path is
# ----------------------------------------------------------------------------------------------------------------
# masked and full rows of every group size (full: 4, 8, 16, 32, 64, 128, 256 = G 1 ... 64), then (64, 2) and (64, 4)
STEP_DIMS = (2, 4, 5, 8, 16, 17, 32, 64, 100, 128, 256, 260, 1024)


def _step_inputs(name, dim):
    return lc.inputs(name, dim, 1.0, salt=11), (1e-4 if name == "rosenbrock" else 1e-3)


@pytest.mark.parametrize("sampler", ["langevin", "heun"])
@pytest.mark.parametrize("name", lc.ENERGIES)
def test_one_noise_free_langevin_step(cuda_device, name, sampler):
    a32, a64 = lc.Adapter(name), lc.Adapter(name, f64=True)
    for dim in STEP_DIMS:
        x0, eta = _step_inputs(name, dim)
        case = Case(sampler, name, dim, n=x0.shape[0])
        got = run_langevin(case, _spec(name, cuda_device), x0, eta, False, cuda_device).x
        if sampler == "heun":
            r32 = oracle.langevin.heun_step(a32, x0, None, eta, None)
            r64 = oracle.langevin.heun_step(a64, x0.double(), None, eta, None)
        else:
            r32 = oracle.langevin.em_step(x0, a32.grad(x0), None, eta, None)
            r64 = oracle.langevin.em_step(x0.double(), a64.grad(x0), None, eta, None)
        print(yardstick(got, r32, r64, k_med=2.0, k_max=16.0, what=f"{sampler}-{name}-{dim}"))


@pytest.mark.parametrize("name", lc.ENERGIES)
def test_one_descent_step(cuda_device, name):
    a32, a64 = lc.Adapter(name), lc.Adapter(name, f64=True)
    for dim in STEP_DIMS:
        x0, eta = _step_inputs(name, dim)
        n = x0.shape[0]
        x = x0.to(cuda_device).clone()
        _lib.call("ebm_descent_chain_f32", _spec(name, cuda_device).to_c(), x.data_ptr(), n, dim, 1, eta, None, 0, 0.0, 1, None,
                  _lib.stream_handle(cuda_device))
        r32 = x0 - eta * a32.grad(x0)
        r64 = x0.double() - eta * a64.grad(x0)
        print(yardstick(x.cpu(), r32, r64, k_med=2.0, k_max=16.0, what=f"descent-{name}-{dim}"))


def _mass(kind, dim):
    if kind == "none":
        return None
    if kind == "scalar":
        return 2.5
    g = torch.Generator().manual_seed(dim)
    return torch.rand(dim, generator=g) * 3.0 + 0.5


def _mass64(mass):
    return mass.double() if torch.is_tensor(mass) else mass


@pytest.mark.parametrize("mass_kind", ["none", "scalar", "diag"])
@pytest.mark.parametrize("name", lc.ENERGIES)
def test_one_leapfrog_step_with_injected_momenta(cuda_device, name, mass_kind):
    a32, a64 = lc.Adapter(name), lc.Adapter(name, f64=True)
    for dim in STEP_DIMS:
        x0, eps = _step_inputs(name, dim)
        eps = float(torch.tensor(10 * eps, dtype=torch.float32))
        n = x0.shape[0]
        mass = _mass(mass_kind, dim)
        p = torch.randn(n, dim, generator=torch.Generator().manual_seed(5 + dim))
        u = torch.zeros(n)  # u = 0 accepts every proposal with a > 0: the state returned is the proposal
        case = Case("hmc", name, dim, mass=mass_kind, n=n)
        run = run_hmc(case, _spec(name, cuda_device), x0, p, u, mass, eps, cuda_device)
        assert bool(run.mask.bool().all())
        pm = p if mass is None else p * (math.sqrt(mass) if isinstance(mass, float) else mass.sqrt())
        r32, _ = oracle.hmc.leapfrog(a32, x0, pm, eps, 1, mass, safe=True)
        m64 = _mass64(mass)
        pm64 = p.double() if mass is None else p.double() * (math.sqrt(mass) if isinstance(mass, float) else m64.sqrt())
        r64, _ = oracle.hmc.leapfrog(a64, x0.double(), pm64, eps, 1, m64, safe=True)
        print(yardstick(run.x, r32, r64, k_med=2.0, k_max=16.0, what=f"leapfrog-{name}-{dim}-{mass_kind}"))


# ----------------------------------------------------------------------------------------------------------------
# structure (exact)
# ----------------------------------------------------------------------------------------------------------------
def _chain(spec, x, k, dev, *, eta=1e-4, sigma=1.0, table=None, clamp=None, thin=1, traj=None, noise=None, seed=11, step0=5, heun=False,
           noise_coef=None):
    n, dim = x.shape
    a, sq, coef = em_coefficients(eta, sigma)
    if noise_coef is not None:
        coef = noise_coef
    _lib.call("ebm_langevin_heun_chain_f32" if heun else "ebm_langevin_chain_f32", spec.to_c(), x.data_ptr(), n, dim, k, a, sq, coef,
              None if table is None else table.data_ptr(), 0 if clamp is None else 1, 0.0 if clamp is None else clamp[0],
              0.0 if clamp is None else clamp[1], thin, None if traj is None else traj.data_ptr(), None,
              None if noise is None else noise.data_ptr(), seed, step0, _lib.stream_handle(dev))
    torch.cuda.synchronize()
    return x


STRUCT_DIMS = (5, 8, 16, 32, 64, 100, 128, 256, 257)  # every full group size from 2 lanes up, and masked rows


@pytest.mark.parametrize("name", lc.ENERGIES)
def test_noise_paths_agree_bit_for_bit(cuda_device, name):
    dev = cuda_device
    spec = _spec(name, dev)
    for dim in STRUCT_DIMS:
        x0 = lc.inputs(name, dim, 1.0, n=301, salt=2).to(dev)
        n, k = x0.shape[0], 4
        # an injected all-zero field with noise_coef != 0 is the noise-free call
        free = _chain(spec, x0.clone(), k, dev, noise_coef=0.0)
        zero = _chain(spec, x0.clone(), k, dev, noise=torch.zeros(k, n, dim, device=dev))
        assert torch.equal(free, zero), (name, dim)
        # native noise is ebm_noise_fill_f32's field, injected
        field = torch.empty(k, n, dim, device=dev)
        for i in range(k):  # (a step's slice of the field is 16-byte aligned only where n dim is a multiple of 4: fill a buffer of its own)
            step = torch.empty(n, dim, device=dev)
            _lib.call("ebm_noise_fill_f32", step.data_ptr(), n * dim, _lib.NOISE_NORMAL, 11, 5 + i, _lib.stream_handle(dev))
            field[i] = step
        native = _chain(spec, x0.clone(), k, dev)
        inject = _chain(spec, x0.clone(), k, dev, noise=field)
        assert torch.equal(native, inject), (name, dim)
        assert not torch.equal(native, free)


@pytest.mark.parametrize("name", lc.ENERGIES)
def test_trajectory_table_clamp_and_chain_independence(cuda_device, name):
    dev = cuda_device
    spec = _spec(name, dev)
    for dim in STRUCT_DIMS:
        x0 = lc.inputs(name, dim, 1.0, n=301, salt=4).to(dev)
        n, k, thin = x0.shape[0], 6, 2
        traj = torch.zeros(n, k // thin, dim, device=dev)
        full = _chain(spec, x0.clone(), k, dev, thin=thin, traj=traj)
        for j in range(k // thin):  # row j of a k-step call is the final state of a (j + 1) thin-step call
            part = _chain(spec, x0.clone(), (j + 1) * thin, dev)
            assert torch.equal(traj[:, j], part), (name, dim, j)
        assert torch.equal(traj[:, -1], full)
        # a constant coefficient table is the scalar call
        a, sq, coef = em_coefficients(1e-4, 1.0)
        table = torch.tensor([[a, sq, coef, 0.0]] * k, device=dev)
        assert torch.equal(_chain(spec, x0.clone(), k, dev, table=table), full), (name, dim)
        # clamp clamps
        cl = _chain(spec, x0.clone(), k, dev, clamp=(-0.25, 0.5))
        assert cl.min().item() >= -0.25 and cl.max().item() <= 0.5 and (cl == 0.5).any() and (cl == -0.25).any()
        # the first m chains of an n-chain call are an m-chain call
        m = 77
        assert torch.equal(_chain(spec, x0[:m].clone(), k, dev), full[:m]), (name, dim)
        h_full = _chain(spec, x0.clone(), 3, dev, heun=True)
        assert torch.equal(_chain(spec, x0[:m].clone(), 3, dev, heun=True), h_full[:m]), (name, dim)


@pytest.mark.parametrize("name", lc.ENERGIES)
def test_hmc_chain_independence_and_trajectory(cuda_device, name):
    dev = cuda_device
    spec = _spec(name, dev)
    for dim in STRUCT_DIMS:
        x0 = lc.inputs(name, dim, 0.5, n=301, salt=6)
        n, T, L, m = x0.shape[0], 4, 3, 77
        g = torch.Generator().manual_seed(dim)
        p, u = torch.randn(T, n, dim, generator=g), torch.rand(T, n, generator=g)
        eps = 1e-3
        full = run_hmc(Case("hmc", name, dim, n=n), spec, x0, p, u, None, eps, dev, T=T, L=L, traj=True)
        part = run_hmc(Case("hmc", name, dim, n=m), spec, x0[:m], p[:, :m], u[:, :m], None, eps, dev, T=T, L=L)
        assert torch.equal(part.x, full.x[:m]) and torch.equal(part.mask, full.mask[:, :m]), (name, dim)
        for j in range(T):
            sub = run_hmc(Case("hmc", name, dim, n=n), spec, x0, p[:j + 1], u[:j + 1], None, eps, dev, T=j + 1, L=L)
            assert torch.equal(sub.x, full.traj[:, j]), (name, dim, j)


# ----------------------------------------------------------------------------------------------------------------
# records
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", ["langevin", "heun", "hmc"])
@pytest.mark.parametrize("name", lc.ENERGIES)
def test_records_merge_and_mean_energy(cuda_device, name, sampler):
    dev = cuda_device
    spec = _spec(name, dev)
    m = lc.model(name)
    for dim in (5, 64, 260):
        x0 = lc.inputs(name, dim, 0.5, n=300, salt=8)
        n = x0.shape[0]
        case = Case(sampler, name, dim, records=True, n=n)
        if sampler == "hmc":
            g = torch.Generator().manual_seed(dim)
            p, u = torch.randn(2, n, dim, generator=g), torch.rand(2, n, generator=g)
            run = run_hmc(case, spec, x0, p, u, None, 1e-3, dev, T=2, L=2, thin=2)
        else:
            run = run_langevin(case, spec, x0, 1e-4, True, dev, k=2, thin=2)
        mean, var, energy, acc = diag_finish(run, n, dim, dev, sampler == "hmc")
        mean64, var64, e64, a64 = merge_records64(run.rec, run.layout, n, dim)
        assert torch.allclose(mean.double(), mean64, rtol=1e-6, atol=1e-7), (name, sampler, dim)
        assert torch.allclose(var.double(), var64, rtol=1e-5, atol=1e-10), (name, sampler, dim)
        assert abs(energy.item() - e64.item()) <= 1e-6 * abs(e64.item()) + 1e-7
        # the records speak of the state the call returned: column means exactly, mean energy within the energy bar
        assert torch.allclose(mean64[0], run.x.double().mean(dim=0), rtol=1e-5, atol=1e-6), (name, sampler, dim)
        _, ne = lc.natural(name, m, run.x)
        want = lc.energy64(name, m, run.x).mean().item()
        # the energy bar itself, on the mean: the energy shares of a record are a wave's tree sum of its chains' energies (six
        # levels), each chain's energy is within the bar of its own N_E, and the merge of the records is float64
        bar = lc.BAR[name]["energy"] * lc.U * ne.mean().item()
        print(name, sampler, dim, "mean energy", e64.item(), "float64", want, "bar", bar)
        assert abs(e64.item() - want) <= bar, (name, sampler, dim)
        if sampler == "hmc":
            assert abs(a64.item() - run.mask[-1].float().mean().item()) < 1e-6


# ----------------------------------------------------------------------------------------------------------------
# HMC: accept decisions and safe mode
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lc.ENERGIES)
def test_accept_decisions_follow_float64(cuda_device, name):
    for dim in (2, 17, 64, 260):
        x, p, eps, (h0, h1, n0, n1) = lc.accept_batch(name, dim)
        keep, u, below = accept_draws(h0, h1, n0, n1)
        share = keep.float().mean().item()
        run = run_hmc(Case("hmc", name, dim, n=x.shape[0]), _spec(name, cuda_device), x, p, u, None, eps, cuda_device)
        got = run.mask[0].bool()
        wrong = int((got[keep] != below[keep]).sum())
        print(name, dim, "eps", eps, "kept share %.3f" % share, "kept", int(keep.sum()), "wrong", wrong)
        assert share >= 0.40, (name, dim, share)
        assert wrong == 0, (name, dim, wrong)


def _safe_mode_check(name, x0, eps, T, L, dev):
    """tests/test_hmc_ring_gpu.py::test_safe_mode_literal_sequence_matches_oracle: the same NaN / inf pattern exactly, finite
    values of the wild chains to a relative 1e-3, tame chains to 5e-4, masks equal where the oracle's margin exceeds 2e-4."""
    n, dim = x0.shape
    g = torch.Generator().manual_seed(77)
    p, u = torch.randn(T, n, dim, generator=g), torch.rand(T, n, generator=g)
    ref = oracle.hmc_chain(lc.Adapter(name), x0, p, u, [eps] * T, L, want_margins=True)
    run = run_hmc(Case("hmc", name, dim, n=n), _spec(name, dev), x0, p, u, None, eps, dev, T=T, L=L)
    return ref, run


def _compare_safe(ref, run, wild):
    got, want = run.x, ref["x"]
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.isinf(got), torch.isinf(want))
    fin = torch.isfinite(want)
    rel = (got - want).abs() / want.abs().clamp(min=1.0)
    rel = torch.where(fin, rel, torch.zeros_like(rel))
    tame = ~wild
    print("wild rel max", rel[wild].max().item() if wild.any() else 0.0, "tame rel max", rel[tame].max().item() if tame.any() else 0.0)
    assert (rel[wild] < 1e-3).all() and (rel[tame] < 5e-4).all()
    sure = ref["margins"] > 2e-4
    assert torch.equal(run.mask.bool()[sure], ref["accepted"][sure])


def test_safe_mode_ackley_from_the_origin(cuda_device):
    """E(0) = 0 is finite, the gradient there is NaN: the kernel's check value sends those lane groups to the literal
    sequence (NaN-propagating clamp, scrub, re-evaluated force), as the reference's safe mode runs it."""
    for dim in (4, 20, 260):
        x0 = lc.inputs("ackley", dim, 0.5, n=200, salt=12)
        wild = torch.zeros(200, dtype=torch.bool)
        wild[::3] = True
        x0[wild] = 0.0
        ref, run = _safe_mode_check("ackley", x0, 0.01, 3, 4, cuda_device)
        _compare_safe(ref, run, wild)


def test_safe_mode_rosenbrock_with_an_overflowing_gradient(cuda_device):
    """Starts whose gradient overflows (the clamp then holds the force at +-1e6; inf - inf coordinates are NaN and are
    scrubbed).  In fp32 with the default b the energy overflows with it -- docs/design/landscapes.md, the check value."""
    for dim in (4, 20, 260):
        x0 = lc.inputs("rosenbrock", dim, 0.5, n=200, salt=13)
        wild = torch.zeros(200, dtype=torch.bool)
        wild[::4] = True
        idx = torch.arange(200)
        x0[wild & (idx % 3 == 0), 0] = 1.0e13        # r_0 = -1e26: 4 b x_0 r_0 = -4e41 overflows (and b r_0^2 with it)
        x0[wild & (idx % 3 == 1), dim - 1] = 3.0e19  # r_{n-2} = 3e19: infinite energy, finite gradient
        x0[wild & (idx % 3 == 2), 0] = 1.0e13        # ... and a second large coordinate: infinities of both signs meet
        x0[wild & (idx % 3 == 2), 1] = 1.0e30
        ref, run = _safe_mode_check("rosenbrock", x0, 0.01, 3, 4, cuda_device)
        _compare_safe(ref, run, wild)


# ----------------------------------------------------------------------------------------------------------------
# law: Rastrigin at a = 1 has independent coordinates with density ~ exp(-(x^2 - cos 2 pi x))
# ----------------------------------------------------------------------------------------------------------------
def _rastrigin_cdf():
    import numpy as np

    grid = np.linspace(-8.0, 8.0, 320001)
    dens = np.exp(-(grid ** 2 - np.cos(2 * np.pi * grid)))
    cdf = np.concatenate([[0.0], np.cumsum(0.5 * (dens[1:] + dens[:-1]) * np.diff(grid))])
    cdf /= cdf[-1]
    return lambda v: np.interp(v, grid, cdf)


def test_rastrigin_law_hmc_and_langevin(cuda_device):
    """HMC is exact under Metropolis; unadjusted Langevin is biased at any finite step -- at eps = 2e-3 (eta), k = 4000 a
    float64 chain on the CPU passes the same test, so the kernel must.  Each test looks at ONE coordinate of every chain
    (independent draws)."""
    from scipy import stats

    cdf = _rastrigin_cdf()
    dev = cuda_device
    m = ta.core.RastriginModel(a=1.0, device=dev)
    n, dim = 4000, 4
    x0 = torch.randn(n, dim, generator=torch.Generator().manual_seed(1)).to(dev) * 0.7
    hmc = ta.HamiltonianMonteCarlo(m, step_size=0.15, n_leapfrog_steps=8, device=dev)
    out, diag = hmc.sample(x=x0.clone(), n_steps=300, thin=300, return_diagnostics=True, generator=torch.Generator(device=dev).manual_seed(3))
    rate = diag["acceptance_rate"][-1].item()
    pv = stats.kstest(out[:, 0].cpu().double().numpy(), cdf).pvalue
    print("HMC: T = 300, L = 8, eps = 0.15, acceptance rate %.3f, p = %.4f" % (rate, pv))
    assert 0.3 < rate <= 1.0
    assert pv > P_MIN
    lang = ta.LangevinDynamics(m, step_size=2e-3, device=dev)
    out = lang.sample(x=x0.clone(), n_steps=4000, generator=torch.Generator(device=dev).manual_seed(4))
    pv = stats.kstest(out[:, 1].cpu().double().numpy(), cdf).pvalue
    print("Langevin: k = 4000, eta = 2e-3, p = %.4f" % pv)
    assert pv > P_MIN
