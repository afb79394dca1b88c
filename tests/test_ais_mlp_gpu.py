"""ebm_ais_mlp_chain_f32 on the GPU: the kernel through the C ABI with injected draws against the restatement of ais_cases.py
on the CPU network (decisions, and states and log-weights by the fp64 referee), its native draws against the materialised
Philox fields, its transition at beta = 1 against ebm_hmc_chain_f32, a wild start, AnnealedImportanceSampling.run() with the
``fused_mlp`` opt-in, and log Z of a confining 2-D network against quadrature."""

import copy
import functools
import math

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib, _rng
from helpers import hip_calls
from ais_cases import draw_inputs, f32, restate, sigmoid_betas

pytestmark = pytest.mark.gpu
ENTRY = "ebm_ais_mlp_chain_f32"
SENTINEL = 7.0

# (in_dim, hidden, n, T)
CASES = [
    (2, 64, 257, 3),     # three workgroups' worth of waves plus a one-chain tail; half a Philox counter per chain
    (5, 64, 37, 6),      # the per-element Philox path; a wave with 5 live chains
    (32, 128, 70, 4),
    (33, 64, 37, 4),     # DT = 2 with one live column in the second tile
    (64, 128, 37, 4),
    (70, 64, 37, 3),     # H = 64 at DT = 3
    (100, 128, 37, 3),   # mode 0
    (128, 64, 37, 3),
    (128, 128, 33, 2),   # mode 0
    (8, 128, 1, 12),     # a single chain
    (32, 128, 37, 1),    # the table (0, 1)
]
L_CASES = 3


class _CpuMlpEnergy:
    def __init__(self, model):
        self.model = model

    def energy(self, x):
        return self.model(x).detach()

    def grad(self, x):
        return self.model.gradient(x)


@functools.lru_cache(maxsize=None)
def _net(in_dim, hidden):
    torch.manual_seed(10 + in_dim)
    cpu = ta.MLPEnergy(in_dim, hidden)
    with torch.no_grad():
        for p in cpu.parameters():
            p.mul_(1.2)
    return cpu


def _step_sizes(in_dim, T):
    return tuple(1.1 * (2.0 / in_dim) ** 0.25 * (1.0 - 0.02 * t) for t in range(T))


@functools.lru_cache(maxsize=None)
def _case(in_dim, hidden, n, T):
    """Inputs and both restatements of a case, computed once per session and shared (read-only) by the tests that use it."""
    cpu = _net(in_dim, hidden)
    betas, eps = sigmoid_betas(T), _step_sizes(in_dim, T)
    x0, z, u = draw_inputs(3, n, in_dim, T, 1.0)
    ref32 = restate(_CpuMlpEnergy(cpu), x0, z, u, betas, eps, L_CASES, 1.0, torch.float32)
    ref64 = restate(_CpuMlpEnergy(copy.deepcopy(cpu).double()), x0, z, u, betas, eps, L_CASES, 1.0, torch.float64)
    return {"cpu": cpu, "betas": betas, "eps": eps, "x0": x0, "z": z, "u": u, "ref32": ref32, "ref64": ref64}


def run_kernel(dev, cpu_model, n, betas, eps, L, base_std, *, x0=None, z=None, u=None, seed=0, step0=0):
    """One call of the entry -> dict of CPU tensors: states [n, dim], logw [n], the accept mask [T, n], accept counts [T]."""
    T, dim = len(eps), cpu_model.in_dim
    spec = copy.deepcopy(cpu_model).to(dev).fused_spec()
    assert spec is not None and spec.hmc
    betas_d = betas.to(dev)
    eps_d = torch.tensor(list(eps), dtype=torch.float32, device=dev)
    x = torch.full((n, dim), SENTINEL, device=dev)
    logw = torch.full((n,), SENTINEL, device=dev)
    mask = torch.full((T, n), 7, dtype=torch.uint8, device=dev)
    counts = torch.zeros(T, dtype=torch.int32, device=dev)
    x0_d = None if x0 is None else x0.to(dev).contiguous()
    z_d = None if z is None else z.to(dev).contiguous()
    u_d = None if u is None else u.to(dev).contiguous()
    before = hip_calls(ENTRY)
    _lib.call(ENTRY, spec.to_c(), x.data_ptr(), logw.data_ptr(), n, dim, T, L, betas_d.data_ptr(), eps_d.data_ptr(),
              f32(base_std), f32(1.0 / base_std**2), mask.data_ptr(), counts.data_ptr(), _lib.ptr(x0_d), _lib.ptr(z_d), _lib.ptr(u_d),
              seed, step0, _lib.stream_handle(dev))
    torch.cuda.synchronize()
    assert hip_calls(ENTRY) == before + 1
    x, logw, mask = x.cpu(), logw.cpu(), mask.cpu()
    assert int(mask.max()) <= 1, "a row of the accept mask was not written"
    assert not (x == SENTINEL).any() and not (logw == SENTINEL).any(), "a row of the outputs was not written"
    return {"x": x, "logw": logw, "accepted": mask.bool(), "counts": counts.cpu().long()}


@pytest.mark.parametrize("in_dim,hidden,n,T", CASES)
def test_cases_with_injected_draws(cuda_device, in_dim, hidden, n, T):
    """Bars of the MLP HMC kernel's own test (test_mlp_wide_gpu.py): >= 99 % of the chains decided as the fp32 restatement
    decides them; every chain all of whose fp64 margins exceed 1e-4 decided as fp64 decides it; on those chains states and
    log-weights no further from fp64 than 4 x the fp32 restatement's own error (floor: 4e-6 of the largest reference value)."""
    c = _case(in_dim, hidden, n, T)
    ref32, ref64 = c["ref32"], c["ref64"]
    got = run_kernel(cuda_device, c["cpu"], n, c["betas"], c["eps"], L_CASES, 1.0, x0=c["x0"], z=c["z"], u=c["u"])
    agree = (got["accepted"] == ref32["accepted"]).all(dim=0)
    clear = ref64["margin"].min(dim=0).values > 1e-4
    print(f"dim {in_dim} H {hidden} n {n} T {T}: rejected {int((~got['accepted']).sum())}/{got['accepted'].numel()}"
          f" (fp32 restatement {int((~ref32['accepted']).sum())}), agree {agree.float().mean().item():.4f},"
          f" clear {clear.float().mean().item():.4f}")
    for key in ("x", "logw"):
        ref = ref64[key][clear]
        err_hip = (got[key].double()[clear] - ref).abs().max().item()
        err_torch = (ref32[key].double()[clear] - ref).abs().max().item()
        print(f"  {key}: kernel err {err_hip:.3e}, fp32 restatement err {err_torch:.3e}, max|ref| {ref.abs().max().item():.3e}")
    assert agree.float().mean().item() >= 0.99
    assert clear.float().mean().item() > 0.9  # (a condition on the inputs)
    assert (got["accepted"][:, clear] == ref64["accepted"][:, clear]).all()
    assert torch.equal(got["counts"], got["accepted"].sum(dim=1).long())
    for key in ("x", "logw"):
        ref = ref64[key][clear]
        err_hip = (got[key].double()[clear] - ref).abs().max().item()
        err_torch = (ref32[key].double()[clear] - ref).abs().max().item()
        assert err_hip <= max(4.0 * err_torch, 4e-6 * ref.abs().max().item()), (key, err_hip, err_torch)


def _field(dev, kind, seed, step, n_elem):
    out = torch.empty((n_elem + 3) // 4 * 4, device=dev)
    _lib.call("ebm_noise_fill_f32", out.data_ptr(), n_elem, kind, seed, step, _lib.stream_handle(dev))
    return out[:n_elem].clone()


@pytest.mark.parametrize("in_dim,hidden,n,T", [(5, 64, 37, 6), (40, 128, 70, 4)])
def test_native_draws_are_the_materialised_fields(cuda_device, in_dim, hidden, n, T):
    dev, cpu, betas = cuda_device, _net(in_dim, hidden), sigmoid_betas(T)
    seed, step0 = 0x1234567887654321, 77
    x0 = _field(dev, _lib.NOISE_NORMAL, seed, step0, n * in_dim).view(n, in_dim).cpu()  # (base_std = 1: sigma0 z = z)
    z = torch.stack([_field(dev, _lib.NOISE_NORMAL, seed, step0 + 2 * t - 1, n * in_dim) for t in range(1, T + 1)]).view(T, n, in_dim).cpu()
    u = torch.stack([_field(dev, _lib.NOISE_UNIFORM, seed, step0 + 2 * t, n) for t in range(1, T + 1)]).view(T, n).cpu()
    for factor in (1.0, 1.5):  # (1.5: only if the plain step sizes reject nothing)
        eps = tuple(factor * v for v in _step_sizes(in_dim, T))
        native = run_kernel(dev, cpu, n, betas, eps, L_CASES, 1.0, seed=seed, step0=step0)
        if (~native["accepted"]).any():
            break
    fed = run_kernel(dev, cpu, n, betas, eps, L_CASES, 1.0, x0=x0, z=z, u=u)
    for key in ("x", "logw", "accepted", "counts"):
        assert torch.equal(native[key], fed[key]), key
    assert torch.isfinite(native["logw"]).all() and torch.isfinite(native["x"]).all()
    assert (~native["accepted"]).any(), "no proposal was rejected: the accept uniforms were not exercised"
    # a sub-block of chains run alone (another grid, other lanes) reproduces its rows of the full launch
    lo, hi = n // 3, n // 3 + max(n // 2, 1)
    part = run_kernel(dev, cpu, hi - lo, betas, eps, L_CASES, 1.0, x0=x0[lo:hi], z=z[:, lo:hi], u=u[:, lo:hi])
    assert torch.equal(part["x"], fed["x"][lo:hi]) and torch.equal(part["logw"], fed["logw"][lo:hi])
    assert torch.equal(part["accepted"], fed["accepted"][:, lo:hi])


@pytest.mark.parametrize("in_dim,hidden", [(5, 64), (40, 128)])
def test_at_beta_one_the_transition_is_the_hmc_kernels(cuda_device, in_dim, hidden):
    """The table (0, 1): the one transition runs at beta = 1, where the mix 0 * a + 1 * b is exact -- the final state and the
    decisions are those of one ebm_hmc_chain_f32 transition on the same network, draws and L, bit for bit (at these shapes that
    entry runs the general variant of the same mode), and the weight is E_0(x0) - E(x0)."""
    dev, cpu, (n, L) = cuda_device, _net(in_dim, hidden), (111, 4)
    eps = 6.0 * (2.0 / in_dim) ** 0.25  # (long enough to reject: 25 and 6 of the 111 proposals on the fp64 CPU network)
    g = torch.Generator().manual_seed(21)
    x0 = torch.randn(n, in_dim, generator=g)
    z, u = torch.randn(1, n, in_dim, generator=g), torch.rand(1, n, generator=g)
    got = run_kernel(dev, cpu, n, torch.tensor([0.0, 1.0]), (eps,), L, 1.0, x0=x0, z=z, u=u)
    rows, p_d, u_d = x0.to(dev).clone(), z.to(dev), u.to(dev)
    mask = torch.empty(1, n, dtype=torch.uint8, device=dev)
    spec = copy.deepcopy(cpu).to(dev).fused_spec()
    _lib.call("ebm_hmc_chain_f32", spec.to_c(), rows.data_ptr(), n, in_dim, 1, L, f32(eps), None, 0, 0.0,
              None, 1, None, None, mask.data_ptr(), None, p_d.data_ptr(), u_d.data_ptr(), 0, 0, _lib.stream_handle(dev))
    torch.cuda.synchronize()
    assert torch.equal(mask.cpu().bool(), got["accepted"])
    assert (~got["accepted"]).any() and got["accepted"].any()
    assert torch.equal(rows.cpu(), got["x"])
    want = 0.5 * x0.double().square().sum(dim=1) - copy.deepcopy(cpu).double()(x0.double()).detach()
    assert torch.allclose(got["logw"].double(), want, rtol=1e-5, atol=1e-5)


def test_wild_start_stays_in_its_chain(cuda_device):
    """A NaN coordinate in one chain and a 1e20 coordinate (E_0 = +inf) in another: every other chain's state, weight and
    decisions are bitwise those of the clean run, although the wave the wild chains sit in takes the literal path."""
    dev, (in_dim, hidden, n, T) = cuda_device, (5, 64, 37, 6)
    c = _case(in_dim, hidden, n, T)
    x0 = c["x0"].clone()
    x0[3, 2] = float("nan")
    x0[7, 4] = 1e20
    args = (dev, c["cpu"], n, c["betas"], c["eps"], L_CASES, 1.0)
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
def test_run_with_the_opt_in_is_one_launch_with_the_documented_result(cuda_device):
    dev, (n, dim, T) = cuda_device, (300, 6, 20)
    torch.manual_seed(2)
    model = ta.MLPEnergy(dim, 64, device=dev)
    s = ta.AnnealedImportanceSampling(model, n_temperatures=T, schedule="sigmoid", step_size=0.3, n_leapfrog_steps=4, device=dev)
    assert s._route(dim)[0] == "eager"  # the default
    s.fused_mlp = True
    assert s._route(dim)[0] == "fused_mlp"
    g = torch.Generator(device=dev).manual_seed(5)
    before, before_analytic = hip_calls(ENTRY), hip_calls("ebm_ais_chain_f32")
    r = s.run(n, dim, generator=g)
    assert hip_calls(ENTRY) == before + 1 and hip_calls("ebm_ais_chain_f32") == before_analytic
    assert _rng._get_offset(g) == 4 * (2 * T + 1)
    assert r.samples.shape == (n, dim) and r.samples.is_cuda and r.log_weights.shape == (n,) and r.acceptance_rate.shape == (T,)
    assert torch.isfinite(r.samples).all() and torch.isfinite(r.log_weights).all() and r.n_nonfinite == 0
    assert ((r.acceptance_rate > 0.5) & (r.acceptance_rate <= 1.0)).all(), r.acceptance_rate
    assert math.isfinite(r.log_z) and 1.0 <= r.ess <= n and r.log_z_stderr >= 0.0
    again = s.run(n, dim, generator=torch.Generator(device=dev).manual_seed(5))
    other = s.run(n, dim, generator=torch.Generator(device=dev).manual_seed(6))
    assert torch.equal(again.log_weights, r.log_weights) and torch.equal(again.samples, r.samples)
    assert not torch.equal(other.log_weights, r.log_weights)
    # the same instance without the opt-in: the eager route, neither entry
    s.fused_mlp = False
    assert s._route(dim)[0] == "eager"
    before, before_analytic = hip_calls(ENTRY), hip_calls("ebm_ais_chain_f32")
    e = s.run(16, dim, generator=torch.Generator(device=dev).manual_seed(1))
    assert hip_calls(ENTRY) == before and hip_calls("ebm_ais_chain_f32") == before_analytic
    assert e.samples.shape == (16, dim) and torch.isfinite(e.log_weights).all()
    # a width without kernels stays eager with the opt-in; so does a state of another width than the network's
    odd = ta.AnnealedImportanceSampling(ta.MLPEnergy(8, 96, device=dev), n_temperatures=3, step_size=0.1, device=dev)
    odd.fused_mlp = True
    assert odd._route(8)[0] == "eager"
    s.fused_mlp = True
    assert s._route(dim + 1)[0] == "eager"


# ---------------------------------------------------------------------------------
# the law: log Z against quadrature
# ---------------------------------------------------------------------------------
def _confining_net():
    """A 2-D network whose energy grows linearly in every direction: every outer weight is positive."""
    m = ta.MLPEnergy(2, 64)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        d = torch.randn(64, 2, generator=g)
        m.net[0].weight.copy_(2.0 * d / d.norm(dim=1, keepdim=True))
        m.net[0].bias.copy_(0.3 * torch.randn(64, generator=g))
        m.net[2].weight.copy_(2.0 * torch.rand(64, 64, generator=g) / 64)
        m.net[2].bias.copy_(0.1 * torch.randn(64, generator=g))
        m.net[4].weight.copy_(8.0 * torch.rand(1, 64, generator=g) / 64)
        m.net[4].bias.zero_()
    return m


def _log_z_by_quadrature(model, points=481, half_width=12.0):
    """Trapezoid rule on [-12, 12]^2 in fp64 on the CPU network (2401 points per axis: 1.52484475, the density at the edge
    5e-10; this grid gives the same eight decimals -- the integrand is smooth and has died out at the edge)."""
    net = copy.deepcopy(model).double()
    t = torch.linspace(-half_width, half_width, points, dtype=torch.float64)
    with torch.no_grad():
        rows = [torch.trapezoid(torch.exp(-net(torch.stack([t, torch.full_like(t, v)], dim=1))), t) for v in t.tolist()]
    return math.log(torch.trapezoid(torch.stack(rows), t).item())


def test_log_z_of_a_confining_network_is_the_quadrature_value_on_both_routes(cuda_device):
    """n = 4096 chains, T = 32 linear betas, L = 3, seed 0, on the fused-MLP route and on the CPU eager route:
    |log_z - truth| <= 4.5 log_z_stderr with ess >= n / 8 (the bars of test_ais_gpu.py's law test).  The acceptance is ~0.8:
    an uncorrected transition, a wrong sign in the increment or a missing log Z_0 misses this by many standard errors."""
    cpu = _confining_net()
    truth = _log_z_by_quadrature(cpu)
    assert abs(truth - 1.52484475) <= 1e-4, truth
    n, dim = 4096, 2
    for dev in (cuda_device, torch.device("cpu")):
        model = copy.deepcopy(cpu).to(dev)
        s = ta.AnnealedImportanceSampling(model, n_temperatures=32, schedule="linear", step_size=1.3, n_leapfrog_steps=3,
                                          base_std=1.5, device=dev)
        s.fused_mlp = True
        assert s._route(dim)[0] == ("fused_mlp" if dev.type == "cuda" else "eager")
        before = hip_calls(ENTRY)
        r = s.run(n, dim, generator=torch.Generator(device=dev).manual_seed(0))
        assert hip_calls(ENTRY) == before + (1 if dev.type == "cuda" else 0)
        print(dev.type, "log_z", r.log_z, "truth", truth, "stderr", r.log_z_stderr, "z", (r.log_z - truth) / r.log_z_stderr,
              "ess", r.ess, "acceptance", r.acceptance_rate.mean().item())
        assert r.n_nonfinite == 0
        assert r.ess >= n / 8, r.ess
        assert abs(r.log_z - truth) <= 4.5 * r.log_z_stderr, (r.log_z, truth, r.log_z_stderr)
