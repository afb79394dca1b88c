"""ebm_ais_chain_f32 on the GPU: the kernel through the C ABI with injected draws against the restatement of ais_cases.py
(decisions exactly, states and log-weights by the fp64 yardstick), its native draws against the materialised Philox fields,
its transition at beta = 1 against ebm_hmc_chain_f32, and AnnealedImportanceSampling.run() on top of it."""

import math

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib, _rng
from helpers import hip_calls, yardstick
from ais_cases import (CASES, MARGIN_BAR, case, energy_spec, f32, leapfrog_steps, model_of, oracle_of, sigmoid_betas,
                       step_sizes)

pytestmark = pytest.mark.gpu
ENTRY = "ebm_ais_chain_f32"


def run_kernel(dev, spec, n, dim, betas, eps, L, base_std, *, x0=None, z=None, u=None, seed=0, step0=0):
    """One call of the entry -> dict of CPU tensors: states [n, dim], logw [n], the accept mask [T, n], accept counts [T]."""
    T = len(eps)
    model = model_of(spec, dev)
    betas_d = betas.to(dev)
    eps_d = torch.tensor(list(eps), dtype=torch.float32, device=dev)
    x = torch.full((n, dim), 7.0, device=dev)
    logw = torch.full((n,), 7.0, device=dev)
    mask = torch.full((T, n), 7, dtype=torch.uint8, device=dev)
    counts = torch.zeros(T, dtype=torch.int32, device=dev)
    x0_d = None if x0 is None else x0.to(dev).contiguous()
    z_d = None if z is None else z.to(dev).contiguous()
    u_d = None if u is None else u.to(dev).contiguous()
    before = hip_calls(ENTRY)
    _lib.call(ENTRY, model.fused_spec().to_c(), x.data_ptr(), logw.data_ptr(), n, dim, T, L, betas_d.data_ptr(), eps_d.data_ptr(),
              f32(base_std), f32(1.0 / base_std**2), mask.data_ptr(), counts.data_ptr(), _lib.ptr(x0_d), _lib.ptr(z_d), _lib.ptr(u_d),
              seed, step0, _lib.stream_handle(dev))
    torch.cuda.synchronize()
    assert hip_calls(ENTRY) == before + 1
    mask = mask.cpu()
    assert int(mask.max()) <= 1, "a row of the accept mask was not written"
    return {"x": x.cpu(), "logw": logw.cpu(), "accepted": mask.bool(), "counts": counts.cpu().long()}


@pytest.mark.parametrize("kind,dim,n,T", CASES)
def test_cases_with_injected_draws(cuda_device, kind, dim, n, T):
    c = case(kind, dim, n, T)
    ref32, ref64 = c["ref32"], c["ref64"]
    assert ref64["margin"].min().item() > MARGIN_BAR, c["seed"]
    assert torch.equal(ref32["accepted"], ref64["accepted"])
    if n >= 37 and T >= 3:  # the case exercises both outcomes of the decision
        assert 0 < ref32["accepted"].sum() < ref32["accepted"].numel()
    got = run_kernel(cuda_device, c["spec"], n, dim, c["betas"], c["eps"], c["L"], c["base_std"], x0=c["x0"], z=c["z"], u=c["u"])
    assert torch.equal(got["accepted"], ref32["accepted"])
    assert torch.equal(got["counts"], ref32["accepted"].sum(dim=1).long())
    print(yardstick(got["x"], ref32["x"], ref64["x"], k_med=2.0, what=f"{kind} dim {dim} T {T} states"))
    print(yardstick(got["logw"][:, None], ref32["logw"][:, None], ref64["logw"][:, None], k_med=2.0, what=f"{kind} dim {dim} T {T} logw"))


def _field(dev, kind, seed, step, n_elem):
    out = torch.empty((n_elem + 3) // 4 * 4, device=dev)
    _lib.call("ebm_noise_fill_f32", out.data_ptr(), n_elem, kind, seed, step, _lib.stream_handle(dev))
    return out[:n_elem].clone()


# (kind, dim, n, T, step-size factor, base_std): on the CPU restatement with torch's draws these reject 30 - 45 of 222, 26 - 38 of
# 350 and 6 - 15 of 63 proposals
@pytest.mark.parametrize("kind,dim,n,T,factor,base_std", [
    ("double_well", 5, 37, 6, 1.5, 1.0),
    ("gmm", 32, 70, 5, 1.5, 1.5),
    ("gaussian", 256, 9, 7, 2.0, 0.8),
])
def test_native_draws_are_the_materialised_fields(cuda_device, kind, dim, n, T, factor, base_std):
    dev, spec, L = cuda_device, energy_spec(kind, dim), leapfrog_steps(dim)
    betas, eps = sigmoid_betas(T), tuple(factor * v for v in step_sizes(kind, dim, T))
    seed, step0 = 0x1234567887654321, 77
    native = run_kernel(dev, spec, n, dim, betas, eps, L, base_std, seed=seed, step0=step0)
    x0 = (f32(base_std) * _field(dev, _lib.NOISE_NORMAL, seed, step0, n * dim)).view(n, dim).cpu()
    z = torch.stack([_field(dev, _lib.NOISE_NORMAL, seed, step0 + 2 * t - 1, n * dim) for t in range(1, T + 1)]).view(T, n, dim).cpu()
    u = torch.stack([_field(dev, _lib.NOISE_UNIFORM, seed, step0 + 2 * t, n) for t in range(1, T + 1)]).view(T, n).cpu()
    fed = run_kernel(dev, spec, n, dim, betas, eps, L, base_std, x0=x0, z=z, u=u)
    for key in ("x", "logw", "accepted", "counts"):
        assert torch.equal(native[key], fed[key]), key
    assert torch.isfinite(native["logw"]).all() and torch.isfinite(native["x"]).all()
    assert (~native["accepted"]).any(), "no proposal was rejected: the accept uniforms were not exercised"
    # a sub-block of chains run alone (another grid, other lanes) reproduces its rows of the full launch
    lo, hi = n // 3, n // 3 + max(n // 2, 1)
    part = run_kernel(dev, spec, hi - lo, dim, betas, eps, L, base_std, x0=x0[lo:hi], z=z[:, lo:hi], u=u[:, lo:hi])
    assert torch.equal(part["x"], fed["x"][lo:hi]) and torch.equal(part["logw"], fed["logw"][lo:hi])
    assert torch.equal(part["accepted"], fed["accepted"][:, lo:hi])


@pytest.mark.parametrize("dim", [5, 100])
def test_at_beta_one_the_transition_is_the_hmc_kernels(cuda_device, dim):
    """The table (0, 1): the one transition runs at beta = 1, where the mix 0 * a + 1 * b is exact -- the final state is that of
    one ebm_hmc_chain_f32 transition, bit for bit (double well at dims where that entry runs the lane-group kernel of the same
    geometry), and the weight is E_0(x0) - E(x0)."""
    dev, (n, L, eps) = cuda_device, (111, 4, 0.15)
    spec = energy_spec("double_well", dim)
    g = torch.Generator().manual_seed(21)
    x0 = torch.randn(n, dim, generator=g)
    z, u = torch.randn(1, n, dim, generator=g), torch.rand(1, n, generator=g)
    got = run_kernel(dev, spec, n, dim, torch.tensor([0.0, 1.0]), (eps,), L, 1.0, x0=x0, z=z, u=u)
    rows, p_d, u_d = x0.to(dev).clone(), z.to(dev), u.to(dev)
    mask = torch.empty(1, n, dtype=torch.uint8, device=dev)
    _lib.call("ebm_hmc_chain_f32", model_of(spec, dev).fused_spec().to_c(), rows.data_ptr(), n, dim, 1, L, eps, None, 0, 0.0,
              None, 1, None, None, mask.data_ptr(), None, p_d.data_ptr(), u_d.data_ptr(), 0, 0, _lib.stream_handle(dev))
    torch.cuda.synchronize()
    assert torch.equal(mask.cpu().bool(), got["accepted"])
    assert (~got["accepted"]).any() and got["accepted"].any()
    assert torch.equal(rows.cpu(), got["x"])
    want = 0.5 * x0.double().square().sum(dim=1) - oracle_of(spec).energy(x0.double())
    assert torch.allclose(got["logw"].double(), want, rtol=1e-5, atol=1e-5)


def test_wild_start_stays_in_its_chain(cuda_device):
    """A NaN coordinate in one chain and a 1e20 coordinate (a +inf energy) in another: every other chain's state, weight and
    decisions are bitwise those of the clean run."""
    dev, (kind, dim, n, T) = cuda_device, ("double_well", 5, 37, 6)
    c = case(kind, dim, n, T)
    x0 = c["x0"].clone()
    x0[3, 2] = float("nan")
    x0[7, 4] = 1e20  # x^2 overflows: the energy is +inf
    assert torch.isinf(oracle_of(c["spec"]).energy(x0[7:8])).all()
    args = (dev, c["spec"], n, dim, c["betas"], c["eps"], c["L"], c["base_std"])
    got = run_kernel(*args, x0=x0, z=c["z"], u=c["u"])
    clean = run_kernel(*args, x0=c["x0"], z=c["z"], u=c["u"])
    others = [i for i in range(n) if i not in (3, 7)]
    assert torch.isfinite(clean["x"]).all() and torch.isfinite(clean["logw"]).all()
    assert torch.equal(got["x"][others], clean["x"][others]) and torch.equal(got["logw"][others], clean["logw"][others])
    assert torch.equal(got["accepted"][:, others], clean["accepted"][:, others])
    assert not torch.isfinite(got["logw"][[3, 7]]).any()


# ---------------------------------------------------------------------------------
# through run()
# ---------------------------------------------------------------------------------
def test_run_is_one_launch_with_the_documented_result(cuda_device):
    dev, (n, dim, T) = cuda_device, (300, 6, 20)
    s = ta.AnnealedImportanceSampling(ta.DoubleWellModel(device=dev), n_temperatures=T, schedule="sigmoid", step_size=0.15,
                                      n_leapfrog_steps=4, device=dev)
    assert s._route(dim)[0] == "fused"
    g = torch.Generator(device=dev).manual_seed(5)
    before = hip_calls(ENTRY)
    r = s.run(n, dim, generator=g)
    assert hip_calls(ENTRY) == before + 1
    assert _rng._get_offset(g) == 4 * (2 * T + 1)
    assert r.samples.shape == (n, dim) and r.samples.is_cuda and r.log_weights.shape == (n,) and r.acceptance_rate.shape == (T,)
    assert torch.isfinite(r.samples).all() and torch.isfinite(r.log_weights).all() and r.n_nonfinite == 0
    assert ((r.acceptance_rate > 0.5) & (r.acceptance_rate <= 1.0)).all(), r.acceptance_rate
    assert math.isfinite(r.log_z) and 1.0 <= r.ess <= n and r.log_z_stderr >= 0.0
    again = s.run(n, dim, generator=torch.Generator(device=dev).manual_seed(5))
    other = s.run(n, dim, generator=torch.Generator(device=dev).manual_seed(6))
    assert torch.equal(again.log_weights, r.log_weights) and torch.equal(again.samples, r.samples)
    assert not torch.equal(other.log_weights, r.log_weights)
    ll = s.log_likelihood(r.samples[:10], r)
    assert ll.shape == (10,) and torch.allclose(ll, -ta.DoubleWellModel(device=dev)(r.samples[:10]) - r.log_z)


def test_other_configurations_take_the_eager_route_on_the_gpu(cuda_device):
    dev = cuda_device

    class Quartic(ta.BaseModel):
        def forward(self, x):
            return (x**4).sum(dim=-1)

    before = hip_calls(ENTRY)
    for s, dim in [
        (ta.AnnealedImportanceSampling(ta.DoubleWellModel(device=dev), n_temperatures=3, step_size=0.02, device=dev), 300),
        (ta.AnnealedImportanceSampling(Quartic(device=dev), n_temperatures=3, step_size=0.1, device=dev), 4),
        (ta.AnnealedImportanceSampling(ta.MLPEnergy(4, 64, device=dev), n_temperatures=3, step_size=0.1, device=dev), 4),
    ]:
        assert s._route(dim)[0] == "eager"
        r = s.run(16, dim, generator=torch.Generator(device=dev).manual_seed(1))
        assert r.samples.shape == (16, dim) and r.samples.is_cuda and torch.isfinite(r.log_weights).all()
        assert r.acceptance_rate.shape == (3,) and r.acceptance_rate.is_cuda
    assert hip_calls(ENTRY) == before


# ---------------------------------------------------------------------------------
# the law: log Z against the truth
# ---------------------------------------------------------------------------------
def _double_well_log_z(h, b, dim):
    x = torch.linspace(-6.0, 6.0, 200001, dtype=torch.float64)
    return dim * math.log(torch.trapezoid(torch.exp(-h * (x * x - b) ** 2), x).item())


def _rastrigin_log_z(a, dim):
    x = torch.linspace(-8.0, 8.0, 320001, dtype=torch.float64)
    return dim * math.log(torch.trapezoid(torch.exp(-(a + x * x - a * torch.cos(2.0 * math.pi * x))), x).item())


LAW = {
    "harmonic": (lambda dev: ta.HarmonicModel(k=4.0, device=dev), 8, 1.0, 0.35, 4.0 * math.log(2.0 * math.pi / 4.0)),
    "double_well": (lambda dev: ta.DoubleWellModel(barrier_height=2.0, b=1.0, device=dev), 4, 1.0, 0.15, _double_well_log_z(2.0, 1.0, 4)),
    # a landscape kind (the lane-group energies of csrc/landscape_energies.h): independent coordinates, so the truth is one
    # integral.  The CPU eager route alone meets the ess bar at T = 32 (ess 3754 of 4096, z = 0.22)
    "rastrigin": (lambda dev: ta.core.RastriginModel(a=1.0, device=dev), 4, 0.7, 0.15, _rastrigin_log_z(1.0, 4)),
    "ring": (lambda dev: ta.core.ring_mixture(8, 5, radius=3.0, sigma=0.5, device=dev), 5, 2.5, 0.3, 2.5 * math.log(2.0 * math.pi * 0.25)),
}


@pytest.mark.parametrize("target", sorted(LAW))
def test_log_z_is_the_truth_on_both_routes(cuda_device, target):
    """n = 4096 chains, T = 32 linear betas, L = 3, a fixed seed, on the fused route and on the CPU eager route:
    |log_z - truth| <= 4.5 log_z_stderr, with ess >= n / 8 so that the bar cannot go slack.  A missing log Z_0, a wrong sign in
    the increment or an uncorrected transition misses this by many standard errors."""
    make, dim, base_std, eps, truth = LAW[target]
    n = 4096
    for dev in (cuda_device, torch.device("cpu")):
        s = ta.AnnealedImportanceSampling(make(dev), n_temperatures=32, schedule="linear", step_size=eps, n_leapfrog_steps=3,
                                          base_std=base_std, device=dev)
        assert s._route(dim)[0] == ("fused" if dev.type == "cuda" else "eager")
        r = s.run(n, dim, generator=torch.Generator(device=dev).manual_seed(0))
        print(target, dev.type, "log_z", r.log_z, "truth", truth, "stderr", r.log_z_stderr, "z", (r.log_z - truth) / r.log_z_stderr,
              "ess", r.ess, "acceptance", r.acceptance_rate.mean().item())
        assert r.n_nonfinite == 0
        assert r.ess >= n / 8, r.ess
        assert abs(r.log_z - truth) <= 4.5 * r.log_z_stderr, (r.log_z, truth, r.log_z_stderr)
