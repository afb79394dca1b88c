"""ebm_chain_moments_mlp_f32 on the GPU: the kernels through the C ABI with injected draws -- the accumulators against the fp32
recurrence on the entry's own trajectories bit for bit, the walk against the fp64 restatements of langevin_moments_mlp_cases.py --,
what a call writes and what it does not, its native draws against the materialised Philox fields, a sub-block of chains, a call cut
in two, a wild start, a call without energies, the refusals with real buffers, LangevinDynamics.sample_moments() with the opt-in,
and the law of a confining 2-D network against the CPU eager route."""

import copy
import math

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib, _rng
from helpers import hip_calls
from kinetic_mlp_cases import net as flat_net
from langevin_moments_mlp_cases import CASES, ETA, SIGMA, case, coefficients, moments_of, recip_table

pytestmark = pytest.mark.gpu
ENTRY = "ebm_chain_moments_mlp_f32"
ANALYTIC = "ebm_chain_moments_f32"
PLAIN = "ebm_langevin_chain_f32"
FILL = 7.0
GUARD = 64  # elements behind every buffer that must keep their fill


def _guarded(dev, shape, src=None, fill=FILL):
    """A tensor of `shape` holding `fill` (or `src`) in front of GUARD elements of FILL, in one allocation -> (tensor, guard)."""
    numel = 1
    for s in shape:
        numel *= s
    buf = torch.full((numel + GUARD,), FILL, device=dev)
    t = buf[:numel].view(shape)
    t.fill_(fill)
    if src is not None:
        t.copy_(src)
    return t, buf[numel:]


def _spec(dev, cpu_model):
    spec = copy.deepcopy(cpu_model).to(dev).fused_spec()
    assert spec is not None
    return spec


def run_entry(dev, cpu_model, x0, k, burn_in, *, eta=ETA, sigma=SIGMA, noise=None, trajs=True, energy=True, e_traj=None, prefill=FILL,
              seed=0, offset=0):
    """One call of the entry -> dict of CPU tensors: x [n, dim], mom [4, n, dim], e_mom [4, n], traj [n, 2 h, dim], e_traj [n, 2 h].
    Every buffer starts from a fill and sits in front of a guard: a slot the call did not write keeps it, and so must the guards.
    `prefill`: what mom and e_mom hold before the call (the contract: never read at c == 1).  `e_traj`: overrides `trajs` for it."""
    n, dim = x0.shape
    h = (k - burn_in) // 2
    spec = _spec(dev, cpu_model)
    recip = recip_table(h).to(dev)
    bufs = {"x": _guarded(dev, (n, dim), x0), "mom": _guarded(dev, (4, n, dim), fill=prefill)}
    if energy:
        bufs["e_mom"] = _guarded(dev, (4, n), fill=prefill)
    if trajs:
        bufs["traj"] = _guarded(dev, (n, 2 * h, dim))
    if trajs if e_traj is None else e_traj:
        bufs["e_traj"] = _guarded(dev, (n, 2 * h))
    p = lambda key: _lib.ptr(bufs[key][0]) if key in bufs else None  # noqa: E731
    z_d = None if noise is None else noise.to(dev).contiguous()
    a, sq, coef = coefficients(eta, sigma)
    before = hip_calls(ENTRY)
    _lib.call(ENTRY, spec.to_c(), p("x"), n, dim, 0, k, burn_in, a, sq, coef, 0, 0.0, _lib.ptr(recip), p("mom"), p("e_mom"), p("traj"),
              p("e_traj"), None, None, _lib.ptr(z_d), None, seed, offset, _lib.stream_handle(dev))
    torch.cuda.synchronize()
    assert hip_calls(ENTRY) == before + 1
    for key, (_, guard) in bufs.items():
        assert bool((guard == FILL).all()), f"the call wrote behind {key}"
    return {key: t.cpu() for key, (t, _) in bufs.items()}


def run_plain(dev, cpu_model, x0, k, *, eta=ETA, sigma=SIGMA, noise=None, seed=0, offset=0):
    """ebm_langevin_chain_f32 on the same inputs, no clamp -> x."""
    n, dim = x0.shape
    spec = _spec(dev, cpu_model)
    x = x0.to(dev).contiguous().clone()
    z_d = None if noise is None else noise.to(dev).contiguous()
    a, sq, coef = coefficients(eta, sigma)
    _lib.call(PLAIN, spec.to_c(), x.data_ptr(), n, dim, k, a, sq, coef, None, 0, 0.0, 0.0, 1, None, None, _lib.ptr(z_d), seed, offset,
              _lib.stream_handle(dev))
    torch.cuda.synchronize()
    return x.cpu()


# ---------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("in_dim,hidden,n,k,burn_in", CASES)
def test_cases_with_injected_draws(cuda_device, in_dim, hidden, n, k, burn_in):
    """mom and e_mom: the fp32 recurrence on the entry's own traj / e_traj, bit for bit; NULL traj / e_traj and a NaN pre-fill of
    the planes change nothing; x, traj and e_traj no further from fp64 than max(4 x the fp32 restatement's own max error,
    4e-6 x max |ref|), the bar of the sibling MLP tests.  Measured on an MI355X (kernel error / fp32 restatement error per case,
    and whether x equals ebm_langevin_chain_f32's bit for bit): docs/design/langevin_moments_mlp.md."""
    dev, c = cuda_device, case(in_dim, hidden, n, k, burn_in)
    h = c["half"]
    run = lambda **kw: run_entry(dev, c["cpu"], c["x0"], k, burn_in, noise=c["noise"], **kw)  # noqa: E731
    got = run()
    assert got["traj"].shape == (n, 2 * h, in_dim) and got["e_traj"].shape == (n, 2 * h)
    for key in ("x", "mom", "e_mom", "traj", "e_traj"):
        assert not bool((got[key] == FILL).any()), f"a slot of {key} was not written"
    mom, e_mom = moments_of(got["traj"], got["e_traj"], h)
    assert torch.equal(got["mom"], mom), "mom"
    assert torch.equal(got["e_mom"], e_mom), "e_mom"
    assert torch.equal(got["traj"][:, -1], got["x"])
    lean = run(trajs=False)
    assert "traj" not in lean and "e_traj" not in lean
    poisoned = run(prefill=float("nan"))
    for key in ("x", "mom", "e_mom"):
        assert torch.equal(lean[key], got[key]), ("no trajectories", key)
    for key in ("x", "mom", "e_mom", "traj", "e_traj"):
        assert torch.equal(poisoned[key], got[key]), ("NaN pre-fill", key)
    # a finding, not a bar: is the walk ebm_langevin_chain_f32's bit for bit?
    plain = run_plain(dev, c["cpu"], c["x0"], k, noise=c["noise"])
    tag = f"langevin dim {in_dim} H {hidden} n {n} k {k} burn_in {burn_in}"
    print(f"{tag}: x equals {PLAIN}'s bit for bit: {torch.equal(got['x'], plain)} (max |diff| {(got['x'] - plain).abs().max().item():.3e})")
    figures = {}
    for key in ("x", "traj", "e_traj"):
        ref = c["ref64"][key]
        err_hip = (got[key].double() - ref).abs().max().item()
        err_torch = (c["ref32"][key].double() - ref).abs().max().item()
        figures[key] = (err_hip, err_torch, ref.abs().max().item())
        print(f"{tag}: {key} kernel err {err_hip:.3e}, fp32 restatement err {err_torch:.3e} ({err_hip / max(err_torch, 1e-30):.2f} x), "
              f"max|ref| {figures[key][2]:.3e}")
    for key, (err_hip, err_torch, scale) in figures.items():
        assert err_hip <= max(4.0 * err_torch, 4e-6 * scale), (key, err_hip, err_torch, scale)


def test_a_call_without_energies(cuda_device):
    """e_mom = e_traj = NULL (k evaluations, none behind the last step) gives the x, mom and traj of a call with energies; e_traj
    alone is written without e_mom."""
    dev, c = cuda_device, case(5, 128, 37, 11, 3)
    got = run_entry(dev, c["cpu"], c["x0"], 11, 3, noise=c["noise"])
    bare = run_entry(dev, c["cpu"], c["x0"], 11, 3, noise=c["noise"], energy=False, trajs=False)
    assert set(bare) == {"x", "mom"}
    with_traj = run_entry(dev, c["cpu"], c["x0"], 11, 3, noise=c["noise"], energy=False, e_traj=False)
    assert set(with_traj) == {"x", "mom", "traj"}
    only_e_traj = run_entry(dev, c["cpu"], c["x0"], 11, 3, noise=c["noise"], energy=False, trajs=False, e_traj=True)
    assert set(only_e_traj) == {"x", "mom", "e_traj"}
    for other in (bare, with_traj, only_e_traj):
        for key in other:
            assert torch.equal(other[key], got[key]), key


# ---------------------------------------------------------------------------------
# native draws, a sub-block, a call cut in two
# ---------------------------------------------------------------------------------
def _field(dev, seed, step, n_elem):
    out = torch.empty((n_elem + 3) // 4 * 4, device=dev)
    _lib.call("ebm_noise_fill_f32", out.data_ptr(), n_elem, _lib.NOISE_NORMAL, seed, step, _lib.stream_handle(dev))
    return out[:n_elem].clone()


def _fields(dev, seed, offset, n, dim, k):
    """z of a call at (seed, offset): the normal field at step offset + s, element chain * dim + col."""
    return torch.stack([_field(dev, seed, offset + s, n * dim) for s in range(k)]).view(k, n, dim).cpu()


@pytest.mark.parametrize("in_dim,hidden,n", [(5, 64, 37), (33, 128, 70), (40, 128, 37), (128, 64, 70)])
def test_native_draws_are_the_materialised_fields(cuda_device, in_dim, hidden, n):
    """Per-element dims (5, 33) and per-quad ones (40, 128); a sub-block of chains run alone reproduces its rows; a call cut in
    two -- (k1, offset) then (k2, offset + k1), the second piece's burn-in 0 and the first piece's covering it -- reproduces one
    call's x, with injected noise and with native draws."""
    dev, (k, burn_in) = cuda_device, (7, 3)
    cpu = flat_net(in_dim, hidden)
    x0 = torch.randn(n, in_dim, generator=torch.Generator().manual_seed(5))
    seed, offset = 0x1234567887654321, 77
    z = _fields(dev, seed, offset, n, in_dim, k)
    native = run_entry(dev, cpu, x0, k, burn_in, seed=seed, offset=offset)
    fed = run_entry(dev, cpu, x0, k, burn_in, noise=z)
    for key in fed:
        assert torch.equal(native[key], fed[key]), key
        assert torch.isfinite(native[key]).all(), key
    lo, hi = n // 3, n // 3 + max(n // 2, 1)
    part = run_entry(dev, cpu, x0[lo:hi], k, burn_in, noise=z[:, lo:hi])
    for key in ("x", "traj", "e_traj"):
        assert torch.equal(part[key], fed[key][lo:hi]), key
    for key in ("mom", "e_mom"):
        assert torch.equal(part[key], fed[key][:, lo:hi]), key
    # cut in two: 11 steps with the first 5 burnt, as 5 steps (one burnt: a call counts at least four) and 6 steps, none burnt
    k1, k2 = 5, 6
    z_long = _fields(dev, seed, offset, n, in_dim, k1 + k2)
    for fed_noise in (True, False):
        kw = (lambda lo_, hi_: dict(noise=z_long[lo_:hi_])) if fed_noise else (lambda lo_, hi_: dict(seed=seed, offset=offset + lo_))
        whole = run_entry(dev, cpu, x0, k1 + k2, k1, **kw(0, k1 + k2))
        first = run_entry(dev, cpu, x0, k1, 1, **kw(0, k1))
        second = run_entry(dev, cpu, first["x"], k2, 0, **kw(k1, k1 + k2))
        assert torch.equal(second["x"], whole["x"]), ("injected" if fed_noise else "native")
        # the second piece counts the steps the whole call counts: its statistics are the whole call's
        for key in ("mom", "e_mom", "traj", "e_traj"):
            assert torch.equal(second[key], whole[key]), key


# ---------------------------------------------------------------------------------
# non-finite inputs
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 128, 37, 11, 3), (32, 64, 129, 7, 3), (100, 64, 129, 4, 0)])
def test_wild_start_stays_in_its_chain(cuda_device, shape):
    """A NaN coordinate in one chain and a 1e20 coordinate in another, both in the first wave: every other chain's outputs are
    bitwise the clean run's."""
    dev, c = cuda_device, case(*shape)
    run = lambda x0: run_entry(dev, c["cpu"], x0, shape[3], shape[4], noise=c["noise"])  # noqa: E731
    x0 = c["x0"].clone()
    x0[3, 2] = float("nan")
    x0[7, 4] = 1e20
    got, clean = run(x0), run(c["x0"])
    others = [i for i in range(shape[2]) if i not in (3, 7)]
    assert not torch.isfinite(got["x"][3]).all()
    for key in ("x", "traj", "e_traj"):
        assert torch.isfinite(clean[key]).all()
        assert torch.equal(got[key][others], clean[key][others]), key
    for key in ("mom", "e_mom"):
        assert torch.isfinite(clean[key]).all()
        assert torch.equal(got[key][:, others], clean[key][:, others]), key


# ---------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------
def test_refusals_launch_nothing(cuda_device):
    """The refusals of test_langevin_moments_mlp.py with real buffers: each raises its code and no buffer is touched."""
    from test_langevin_moments_mlp import EINVAL, _abi_call

    dev, (n, dim) = cuda_device, (4, 8)
    names = ("x", "recip", "mom", "e_mom", "traj", "e_traj", "noise")
    bufs = {name: torch.full((4 * n * 132,), FILL, device=dev) for name in names}
    real = {name: bufs[name].data_ptr() for name in names}
    desc = ta.MLPEnergy(dim, 64, device=dev).fused_spec().to_c()
    for kw, match in EINVAL:
        with pytest.raises(ValueError, match=match):
            _abi_call(desc, **{**real, **kw})
    with pytest.raises(ValueError, match="bad shape"):
        _abi_call(desc, n=-1, **real)
    for key in ("x", "mom", "traj", "noise"):
        with pytest.raises(ValueError, match="16-byte aligned"):
            _abi_call(desc, **{**real, key: real[key] + 4})
    with pytest.raises(ValueError, match="energy descriptor is NULL"):
        _abi_call(None, **real)
    with pytest.raises(RuntimeError, match=r"code -2.*MLP energy only"):
        _abi_call(ta.DoubleWellModel(device=dev).fused_spec().to_c(), **real)
    with pytest.raises(RuntimeError, match=r"code -2.*MLP energy only"):
        _abi_call(ta.GaussianModel(torch.zeros(dim), torch.eye(dim), device=dev).fused_spec().to_c(), **real)
    with pytest.raises(RuntimeError, match=r"code -2.*no running-moments kernel"):
        _abi_call(desc, entry=ANALYTIC, **real)
    with pytest.raises(RuntimeError, match=r"code -3.*got 64, 129"):
        _abi_call(desc, dim=129, **real)
    with pytest.raises(RuntimeError, match=r"code -3.*got 64, 0"):
        _abi_call(desc, dim=0, **real)
    wide = ta.MLPEnergy(dim, 64, device=dev).fused_spec().to_c()
    wide.n_comp = 96
    with pytest.raises(RuntimeError, match=r"code -3.*got 96, 8"):
        _abi_call(wide, **real)
    torch.cuda.synchronize()
    for name, t in bufs.items():
        assert bool((t == FILL).all()), name


# ---------------------------------------------------------------------------------
# through the sampler
# ---------------------------------------------------------------------------------
def test_sample_moments_with_the_opt_in_is_one_launch(cuda_device):
    dev, (n, dim, k, burn_in) = cuda_device, (300, 6, 11, 3)
    cpu = flat_net(dim, 64)
    model = copy.deepcopy(cpu).to(dev)
    x0 = torch.randn(n, dim, device=dev)
    keep = x0.clone()
    s = ta.LangevinDynamics(model, step_size=ETA, noise_scale=SIGMA, device=dev)
    s.fused_mlp_moments = True
    assert s._route(x0, {})[0] == "fused"
    g = torch.Generator(device=dev).manual_seed(5)
    before = hip_calls(ENTRY), hip_calls(PLAIN), hip_calls(ANALYTIC)
    x, mom = s.sample_moments(x=x0, n_steps=k, burn_in=burn_in, energy=True, generator=g)
    torch.cuda.synchronize()
    assert (hip_calls(ENTRY), hip_calls(PLAIN), hip_calls(ANALYTIC)) == (before[0] + 1, before[1], before[2])
    assert torch.equal(x0, keep), "the caller's tensor was touched"
    assert x.is_cuda and x.shape == (n, dim) and x.data_ptr() != x0.data_ptr()
    # the generator is advanced as by sample()
    g2 = torch.Generator(device=dev).manual_seed(5)
    xs = s.sample(x=x0, n_steps=k, generator=g2)
    assert hip_calls(PLAIN) == before[1] + 1 and _rng._get_offset(g) == _rng._get_offset(g2) == 4 * k
    # ... and x_final is sample()'s draw for draw: equal up to the rounding of two evaluations of the same gradient
    assert torch.allclose(x, xs, rtol=0, atol=1e-4 * float(xs.abs().max()))
    # the moments are the entry's at the generator's coordinates
    want = run_entry(dev, cpu, x0.cpu(), k, burn_in, seed=_rng.kernel_seed(5), offset=0)
    h = (k - burn_in) // 2
    assert mom.half_len == h and mom.n_nonfinite == 0 and mom.acceptance_rate is None
    assert torch.equal(mom.chain_mean.cpu(), want["mom"][[0, 2]]) and torch.equal(mom.chain_m2.cpu(), want["mom"][[1, 3]])
    assert torch.equal(mom.energy_mean.cpu(), want["e_mom"][[0, 2]]) and torch.equal(mom.energy_m2.cpu(), want["e_mom"][[1, 3]])
    assert torch.equal(x.cpu(), want["x"])
    # without energy: the same states and moments
    x2, mom2 = s.sample_moments(x=x0, n_steps=k, burn_in=burn_in, generator=torch.Generator(device=dev).manual_seed(5))
    assert hip_calls(ENTRY) == before[0] + 3  # (run_entry above made one)
    assert torch.equal(x2, x) and torch.equal(mom2.chain_mean, mom.chain_mean) and mom2.energy_mean is None


def test_without_the_opt_in_or_off_its_shapes_the_entry_is_not_launched(cuda_device):
    dev = cuda_device
    before = hip_calls(ENTRY)
    torch.manual_seed(3)
    x0 = torch.randn(32, 6, device=dev)
    gen = lambda: torch.Generator(device=dev).manual_seed(1)  # noqa: E731
    # no opt-in: the step-by-step recurrence, as before
    s = ta.LangevinDynamics(ta.MLPEnergy(6, 64, device=dev), step_size=0.05, device=dev)
    assert s._route(x0, {})[0] == "fused" and s.fused_mlp_moments is False
    x, mom = s.sample_moments(x=x0, n_steps=8, burn_in=2, generator=gen())
    assert x.shape == (32, 6) and torch.isfinite(mom.mean).all()

    def opted(model, **kw):
        s = ta.LangevinDynamics(model, device=dev, **{"step_size": 0.05, **kw})
        s.fused_mlp_moments = True
        return s

    # the opt-in, but a width without kernels / a clamp / a scheduled step size / Heun / an empty batch
    opted(ta.MLPEnergy(6, 96, device=dev)).sample_moments(x=x0, n_steps=4, generator=gen())
    opted(ta.MLPEnergy(6, 64, device=dev), clamp=(-3.0, 3.0)).sample_moments(x=x0, n_steps=4, generator=gen())
    opted(ta.MLPEnergy(6, 64, device=dev), step_size=ta.core.schedules.LinearScheduler(0.05, 0.01, 10)).sample_moments(
        x=x0, n_steps=4, generator=gen())
    opted(ta.MLPEnergy(6, 64, device=dev), integrator="heun").sample_moments(x=x0, n_steps=4, generator=gen())
    opted(ta.MLPEnergy(6, 64, device=dev)).sample_moments(x=x0[:0], n_steps=4, generator=gen())
    # an analytic energy keeps its own one-launch route with the opt-in set
    analytic = hip_calls(ANALYTIC)
    opted(ta.DoubleWellModel(device=dev)).sample_moments(x=x0, n_steps=4, generator=gen())
    assert hip_calls(ANALYTIC) == analytic + 1
    assert hip_calls(ENTRY) == before


# ---------------------------------------------------------------------------------
# the law
# ---------------------------------------------------------------------------------
def _per_chain(mom):
    """Per-chain contributions (float64, CPU) whose means over the chains are the pooled mean and (up to M l / (M l - 1)) the pooled
    variance of ChainMoments: their sample variances over the independent chains give the standard errors."""
    mean, m2 = mom.chain_mean.cpu().double(), mom.chain_m2.cpu().double()
    h = mom.half_len
    m_i = mean.mean(dim=0)  # [n, dim]
    grand = m_i.mean(dim=0)
    s_i = m2.sum(dim=0) / (2 * h) + ((mean - grand) ** 2).mean(dim=0)
    return m_i, s_i


def test_the_law_of_a_confining_network_is_the_eager_routes(cuda_device):
    """The confining 2-D network of test_ais_mlp_gpu.py, n = 4096, step size 0.05, 300 steps of which the first 100 are burnt,
    seed 0, on the one-launch route and on the CPU eager route: the pooled mean and variance of ChainMoments per coordinate differ by
    at most 4.5 standard errors of the difference, the standard errors from the sample variances of the chains' own contributions."""
    from test_ais_mlp_gpu import _confining_net

    cpu = _confining_net()
    n, dim, k, burn_in = 4096, 2, 300, 100
    x0 = torch.randn(n, dim, generator=torch.Generator().manual_seed(0))
    stats = {}
    for dev in (cuda_device, torch.device("cpu")):
        s = ta.LangevinDynamics(copy.deepcopy(cpu).to(dev), step_size=0.05, device=dev)
        s.fused_mlp_moments = True
        before = hip_calls(ENTRY)
        _, mom = s.sample_moments(x=x0.to(dev), n_steps=k, burn_in=burn_in, generator=torch.Generator(device=dev).manual_seed(0))
        assert hip_calls(ENTRY) == before + (1 if dev.type == "cuda" else 0)
        assert mom.n_nonfinite == 0 and mom.half_len == 100
        m_i, s_i = _per_chain(mom)
        scale = 2 * n * 100 / (2 * n * 100 - 1.0)
        assert torch.allclose(m_i.mean(dim=0), mom.mean.cpu(), rtol=0, atol=1e-12)
        assert torch.allclose(scale * s_i.mean(dim=0), mom.var.cpu(), rtol=1e-9)
        stats[dev.type] = {"mean": (mom.mean.cpu(), m_i.std(dim=0) / math.sqrt(n)), "var": (mom.var.cpu(), scale * s_i.std(dim=0) / math.sqrt(n))}
    zs = {}
    for key in stats["cpu"]:
        (m1, se1), (m2, se2) = stats["cuda"][key], stats["cpu"][key]
        zs[key] = (m1 - m2) / torch.sqrt(se1**2 + se2**2)
        print(f"langevin {key}: one launch {m1.tolist()} +- {se1.tolist()}, CPU eager route {m2.tolist()} +- {se2.tolist()}, "
              f"z = {zs[key].tolist()}")
    for key, z in zs.items():
        assert bool((z.abs() <= 4.5).all()), (key, z.tolist())
