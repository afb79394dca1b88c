"""ebm_chain_moments_f32 on the GPU: the accumulators against the fp32 recurrence on the entry's own trajectory (bit for bit,
every kind, both samplers), the dynamics against the restatement of moments_cases.py and against ebm_langevin_chain_f32 /
ebm_hmc_chain_f32, the native draws against the materialised Philox fields, non-finite inputs, the refusals, and
sample_moments() on top of it.  The routing predicate and the refusals also have a counterpart that needs no GPU."""

import math

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib, _rng
from torchebm_amd.samplers.moments import fused_moments_eligible
from helpers import hip_calls, yardstick
from moments_cases import (ELEMENTWISE, ETA, HMC_CASES, LANGEVIN_CASES, MARGIN_BAR, SIGMA, energy_spec, hmc_case, hmc_step,
                           langevin_case, model_of, recip_table, welford)

gpu = pytest.mark.gpu
ENTRY = "ebm_chain_moments_f32"
LANGEVIN, HMC = 0, 1
FILL = 7.0


def run_entry(dev, spec, sampler, x0, k, burn_in, *, eta=ETA, sigma=SIGMA, eps=0.0, L=0, noise=None, u=None, traj=True, energy=True,
              seed=0, offset=0):
    """One call of the entry -> dict of CPU tensors: x [n, dim], mom [4, n, dim], e_mom [4, n], traj [n, 2 h, dim], e_traj [n, 2 h],
    the accept mask [k, n] and the accept counts [k] (HMC).  Outputs start from FILL: a slot the call did not write keeps it."""
    n, dim = x0.shape
    h = (k - burn_in) // 2
    model = model_of(spec, dev)
    x = x0.to(dev).contiguous().clone()
    recip = recip_table(h).to(dev)
    mom = torch.full((4, n, dim), FILL, device=dev)
    e_mom = torch.full((4, n), FILL, device=dev) if energy else None
    tr = torch.full((n, 2 * h, dim), FILL, device=dev) if traj else None
    e_tr = torch.full((n, 2 * h), FILL, device=dev) if (traj and energy) else None
    mask = torch.full((k, n), 7, dtype=torch.uint8, device=dev) if sampler == HMC else None
    counts = torch.zeros(k, dtype=torch.int32, device=dev) if sampler == HMC else None
    noise_d = None if noise is None else noise.to(dev).contiguous()
    u_d = None if u is None else u.to(dev).contiguous()
    a, sq, coef = eta, eta**0.5, (2.0 * sigma**2) ** 0.5
    before = hip_calls(ENTRY)
    _lib.call(ENTRY, model.fused_spec().to_c(), x.data_ptr(), n, dim, sampler, k, burn_in, a, sq, coef, L, eps, recip.data_ptr(),
              mom.data_ptr(), _lib.ptr(e_mom), _lib.ptr(tr), _lib.ptr(e_tr), _lib.ptr(mask), _lib.ptr(counts), _lib.ptr(noise_d),
              _lib.ptr(u_d), seed, offset, _lib.stream_handle(dev))
    torch.cuda.synchronize()
    assert hip_calls(ENTRY) == before + 1
    out = {"x": x.cpu(), "mom": mom.cpu(), "h": h}
    for key, t in (("e_mom", e_mom), ("traj", tr), ("e_traj", e_tr)):
        out[key] = None if t is None else t.cpu()
    if sampler == HMC:
        out["accepted"] = mask.cpu()
        assert int(out["accepted"].max()) <= 1, "a row of the accept mask was not written"
        out["accepted"] = out["accepted"].bool()
        out["counts"] = counts.cpu().long()
    return out


def check_accumulators(got, lean):
    """mom / e_mom are the fp32 recurrence on the entry's own traj / e_traj, bit for bit; `lean`, the same call without the
    trajectory, returns the same x, mom and e_mom."""
    h = got["h"]
    mean, m2 = welford(got["traj"], h)
    want = torch.stack((mean[0], m2[0], mean[1], m2[1]))
    assert torch.equal(got["mom"], want)
    if got["e_mom"] is not None:
        e_mean, e_m2 = welford(got["e_traj"], h)
        assert torch.equal(got["e_mom"], torch.stack((e_mean[0], e_m2[0], e_mean[1], e_m2[1])))
    assert torch.equal(got["traj"][:, -1], got["x"])
    assert torch.equal(lean["x"], got["x"]) and torch.equal(lean["mom"], got["mom"])
    assert (got["e_mom"] is None) == (lean["e_mom"] is None)
    if got["e_mom"] is not None:
        assert torch.equal(lean["e_mom"], got["e_mom"])


# ---------------------------------------------------------------------------------
# accumulators and dynamics, every kind
# ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("energy", [False, True], ids=["plain", "energy"])
@pytest.mark.parametrize("kind,dim,n,k,burn_in", LANGEVIN_CASES)
def test_langevin_cases_with_injected_noise(cuda_device, kind, dim, n, k, burn_in, energy):
    c = langevin_case(kind, dim, n, k, burn_in)
    args = (cuda_device, c["spec"], LANGEVIN, c["x0"], k, burn_in)
    got = run_entry(*args, noise=c["noise"], energy=energy)
    lean = run_entry(*args, noise=c["noise"], energy=energy, traj=False)
    check_accumulators(got, lean)
    ref32, ref64 = c["ref32"], c["ref64"]
    if kind in ELEMENTWISE:
        assert torch.equal(got["x"], ref32["x"]) and torch.equal(got["traj"], ref32["traj"])
    else:  # the factor test_tempering_gpu.py uses for this transition
        print(yardstick(got["x"], ref32["x"], ref64["x"], k_med=1.5, what=f"langevin {kind} dim {dim}"))
    if energy:  # the energies are those of the counted states: the state error times the gradient is far below these bars; an
        # energy filed under another slot or chain is off by its own size
        want = ref64["e_traj"]
        scale = want.abs().clamp(min=1.0)
        tol = 1e-3 if kind in ELEMENTWISE else 1e-2
        assert ((got["e_traj"].double() - want).abs() / scale).max().item() < tol


@gpu
@pytest.mark.parametrize("kind,dim,n,k,burn_in", HMC_CASES)
def test_hmc_cases_with_injected_draws(cuda_device, kind, dim, n, k, burn_in):
    c = hmc_case(kind, dim, n, k, burn_in)
    ref32, ref64 = c["ref32"], c["ref64"]
    assert ref64["margin"].min().item() > MARGIN_BAR, c["seed"]
    args = (cuda_device, c["spec"], HMC, c["x0"], k, burn_in)
    kw = dict(eps=c["eps"], L=c["L"], noise=c["z"], u=c["u"])
    got = run_entry(*args, **kw)
    lean = run_entry(*args, traj=False, **kw)
    check_accumulators(got, lean)
    assert torch.equal(lean["accepted"], got["accepted"]) and torch.equal(lean["counts"], got["counts"])
    assert torch.equal(got["accepted"], ref32["accepted"])
    assert torch.equal(got["counts"], ref32["accepted"].sum(dim=1).long())
    if n >= 37:
        assert 0 < got["accepted"].sum() < got["accepted"].numel()
    # the factor test_ais_gpu.py uses for this transition
    print(yardstick(got["x"], ref32["x"], ref64["x"], k_med=2.0, what=f"hmc {kind} dim {dim}"))
    # (a gross-error check, as for Langevin: an energy filed under another slot or chain is off by its own size)
    want = ref64["e_traj"]
    assert ((got["e_traj"].double() - want).abs() / want.abs().clamp(min=1.0)).max().item() < 1e-2
    # without e_mom the HMC call returns the same states and coordinate moments
    bare = run_entry(*args, traj=False, energy=False, **kw)
    assert bare["e_mom"] is None and torch.equal(bare["x"], got["x"]) and torch.equal(bare["mom"], got["mom"])


# ---------------------------------------------------------------------------------
# against the chain entries
# ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dim", [5, 64])
def test_native_langevin_states_are_the_chain_entrys(cuda_device, dim):
    dev, (n, k, burn_in) = cuda_device, (257, 11, 3)
    spec = energy_spec("double_well", dim)
    x0 = torch.randn(n, dim, generator=torch.Generator().manual_seed(dim))
    seed, offset = 0x0123456789ABCDEF, 41
    got = run_entry(dev, spec, LANGEVIN, x0, k, burn_in, seed=seed, offset=offset, traj=False, energy=False)
    rows = x0.to(dev).clone()
    a, sq, coef = ETA, ETA**0.5, (2.0 * SIGMA**2) ** 0.5
    _lib.call("ebm_langevin_chain_f32", model_of(spec, dev).fused_spec().to_c(), rows.data_ptr(), n, dim, k, a, sq, coef, None, 0, 0.0,
              0.0, 1, None, None, None, seed, offset, _lib.stream_handle(dev))
    torch.cuda.synchronize()
    assert torch.equal(rows.cpu(), got["x"])
    assert not torch.equal(got["x"], x0)


@gpu
@pytest.mark.parametrize("dim", [5, 100])
def test_the_hmc_transition_is_the_hmc_kernels(cuda_device, dim):
    """Double well at dims where ebm_hmc_chain_f32 runs the lane-group kernel of the same geometry: final states and the accept
    mask on the same injected draws, bit for bit."""
    dev, (n, k, L, eps) = cuda_device, (111, 6, 4, 0.15)
    spec = energy_spec("double_well", dim)
    g = torch.Generator().manual_seed(21)
    x0 = torch.randn(n, dim, generator=g)
    z, u = torch.randn(k, n, dim, generator=g), torch.rand(k, n, generator=g)
    got = run_entry(dev, spec, HMC, x0, k, 0, eps=eps, L=L, noise=z, u=u)
    rows, p_d, u_d = x0.to(dev).clone(), z.to(dev), u.to(dev)
    mask = torch.empty(k, n, dtype=torch.uint8, device=dev)
    _lib.call("ebm_hmc_chain_f32", model_of(spec, dev).fused_spec().to_c(), rows.data_ptr(), n, dim, k, L, eps, None, 0, 0.0,
              None, 1, None, None, mask.data_ptr(), None, p_d.data_ptr(), u_d.data_ptr(), 0, 0, _lib.stream_handle(dev))
    torch.cuda.synchronize()
    assert torch.equal(mask.cpu().bool(), got["accepted"])
    assert (~got["accepted"]).any() and got["accepted"].any()
    assert torch.equal(rows.cpu(), got["x"])


# ---------------------------------------------------------------------------------
# native draws
# ---------------------------------------------------------------------------------
def _field(dev, kind, seed, step, n_elem):
    out = torch.empty((n_elem + 3) // 4 * 4, device=dev)
    _lib.call("ebm_noise_fill_f32", out.data_ptr(), n_elem, kind, seed, step, _lib.stream_handle(dev))
    return out[:n_elem].clone()


@gpu
@pytest.mark.parametrize("sampler,kind,dim,n", [(LANGEVIN, "double_well", 5, 37), (LANGEVIN, "gmm", 32, 70), (HMC, "double_well", 5, 37),
                                                (HMC, "gmm", 32, 70), (HMC, "gaussian", 256, 9)])
def test_native_draws_are_the_materialised_fields(cuda_device, sampler, kind, dim, n):
    dev, (k, burn_in) = cuda_device, (11, 3)
    spec = energy_spec(kind, dim)
    x0 = torch.randn(n, dim, generator=torch.Generator().manual_seed(5))
    seed, offset = 0x1234567887654321, 77
    if sampler == LANGEVIN:
        kw = {}
        noise = torch.stack([_field(dev, _lib.NOISE_NORMAL, seed, offset + s, n * dim) for s in range(k)]).view(k, n, dim).cpu()
        u = None
    else:
        eps, L = hmc_step(kind, dim)
        kw = dict(eps=1.5 * eps, L=L)
        noise = torch.stack([_field(dev, _lib.NOISE_NORMAL, seed, offset + 2 * t, n * dim) for t in range(k)]).view(k, n, dim).cpu()
        u = torch.stack([_field(dev, _lib.NOISE_UNIFORM, seed, offset + 2 * t + 1, n) for t in range(k)]).view(k, n).cpu()
    native = run_entry(dev, spec, sampler, x0, k, burn_in, seed=seed, offset=offset, **kw)
    fed = run_entry(dev, spec, sampler, x0, k, burn_in, noise=noise, u=u, **kw)
    keys = ("x", "mom", "e_mom", "traj", "e_traj") + (("accepted", "counts") if sampler == HMC else ())
    for key in keys:
        assert torch.equal(native[key], fed[key]), key
    assert torch.isfinite(native["mom"]).all() and torch.isfinite(native["e_mom"]).all()
    if sampler == HMC and n >= 37:
        assert (~native["accepted"]).any(), "no proposal was rejected: the accept uniforms were not exercised"
    # a sub-block of chains run alone (another grid, other lanes) reproduces its rows of the full launch
    lo, hi = n // 3, n // 3 + max(n // 2, 1)
    part = run_entry(dev, spec, sampler, x0[lo:hi], k, burn_in, noise=noise[:, lo:hi], u=None if u is None else u[:, lo:hi], **kw)
    assert torch.equal(part["x"], fed["x"][lo:hi]) and torch.equal(part["mom"], fed["mom"][:, lo:hi])
    assert torch.equal(part["e_mom"], fed["e_mom"][:, lo:hi]) and torch.equal(part["traj"], fed["traj"][lo:hi])


# ---------------------------------------------------------------------------------
# non-finite inputs
# ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("sampler", [LANGEVIN, HMC])
def test_wild_start_stays_in_its_chain(cuda_device, sampler):
    """A NaN coordinate in one chain and a 1e20 coordinate in another: every other chain's outputs are bitwise the clean run's."""
    dev, (kind, dim, n, k, burn_in) = cuda_device, ("double_well", 5, 37, 11, 3)
    if sampler == LANGEVIN:
        c = langevin_case(kind, dim, n, k, burn_in)
        kw = dict(noise=c["noise"])
    else:
        c = hmc_case(kind, dim, n, k, burn_in)
        kw = dict(eps=c["eps"], L=c["L"], noise=c["z"], u=c["u"])
    x0 = c["x0"].clone()
    x0[3, 2] = float("nan")
    x0[7, 4] = 1e20
    got = run_entry(dev, c["spec"], sampler, x0, k, burn_in, **kw)
    clean = run_entry(dev, c["spec"], sampler, c["x0"], k, burn_in, **kw)
    others = [i for i in range(n) if i not in (3, 7)]
    for key in ("x", "traj", "e_traj"):
        assert torch.isfinite(clean[key]).all()
        assert torch.equal(got[key][others], clean[key][others]), key
    for key in ("mom", "e_mom"):
        assert torch.isfinite(clean[key]).all()
        assert torch.equal(got[key][:, others], clean[key][:, others]), key
    if sampler == HMC:
        assert torch.equal(got["accepted"][:, others], clean["accepted"][:, others])
    assert not torch.isfinite(got["mom"][:, 3]).all()


# ---------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------
def _abi_call(desc, *, x=16, n=4, dim=8, sampler=LANGEVIN, k=8, burn_in=0, L=2, recip=16, mom=16, e_mom=None, noise=None, u=None):
    _lib.call(ENTRY, desc, x, n, dim, sampler, k, burn_in, 0.01, 0.1, 1.4, L, 0.1, recip, mom, e_mom, None, None, None, None, noise, u,
              0, 0, None)


REFUSALS = [
    (dict(dim=257), RuntimeError, r"code -3.*dim 257 > 256"),           # EBM_EDIM: one vector per lane
    (dict(k=7), ValueError, "k_steps=7 burn_in=0"),                      # k_steps - burn_in odd
    (dict(k=8, burn_in=3), ValueError, "k_steps=8 burn_in=3"),
    (dict(k=2), ValueError, "k_steps=2 burn_in=0"),                      # h = 1
    (dict(k=5, burn_in=3), ValueError, "k_steps=5 burn_in=3"),
    (dict(sampler=HMC, noise=16), ValueError, "must be given together"),
    (dict(sampler=HMC, u=16), ValueError, "must be given together"),
    (dict(mom=None), ValueError, "recip / mom is NULL"),
    (dict(recip=None), ValueError, "recip / mom is NULL"),
    (dict(x=None), ValueError, "state pointer is NULL"),
    (dict(sampler=2), ValueError, "sampler=2"),
    (dict(sampler=HMC, L=0), ValueError, "n_leapfrog=0"),
]


def test_abi_refusals_need_no_gpu():
    """Every refusal comes in front of any launch (the pointers below are never dereferenced)."""
    desc = _lib.EnergyDesc()
    desc.kind = _lib.ENERGY_DOUBLE_WELL
    for kw, exc, match in REFUSALS:
        with pytest.raises(exc, match=match):
            _abi_call(desc, **kw)
    desc.kind, desc.dev0 = _lib.ENERGY_MLP, 16
    with pytest.raises(RuntimeError, match=r"code -2.*no running-moments kernel"):  # EBM_EKIND
        _abi_call(desc)
    assert _lib.ABI_VERSION == 9 and ENTRY in _lib.EXPORTS


@gpu
def test_refusals_launch_nothing(cuda_device):
    """The same refusals with real buffers: each raises its code and no output buffer is touched."""
    dev, (n, dim) = cuda_device, (4, 8)
    x = torch.full((n, 260), FILL, device=dev)
    mom = torch.full((4, n, 260), FILL, device=dev)
    e_mom = torch.full((4, n), FILL, device=dev)
    recip = recip_table(4).to(dev)
    draws = torch.zeros(8, n, 260, device=dev)
    real = dict(x=x.data_ptr(), mom=mom.data_ptr(), e_mom=e_mom.data_ptr(), recip=recip.data_ptr())
    desc = model_of(energy_spec("double_well", dim), dev).fused_spec().to_c()
    for kw, exc, match in REFUSALS:
        merged = {**real, **{k_: (draws.data_ptr() if v == 16 and k_ in ("noise", "u") else v) for k_, v in kw.items()}}
        with pytest.raises(exc, match=match):
            _abi_call(desc, **merged)
    mlp = ta.MLPEnergy(dim, 64, device=dev)
    with pytest.raises(RuntimeError, match=r"code -2"):
        _abi_call(mlp.fused_spec().to_c(), **real)
    torch.cuda.synchronize()
    for t in (x, mom, e_mom):
        assert bool((t == FILL).all())


# ---------------------------------------------------------------------------------
# through sample_moments()
# ---------------------------------------------------------------------------------
ELIGIBLE = dict(is_cuda=True, dtype=torch.float32, ndim=2, dim=64, spec_kind=_lib.ENERGY_DOUBLE_WELL, constant=True,
                has_model_kwargs=False, plain_integrator=True, autocast=False, extras_ok=True)


def test_routing_predicate():
    assert fused_moments_eligible(**ELIGIBLE)
    assert fused_moments_eligible(**{**ELIGIBLE, "dim": 256}) and fused_moments_eligible(**{**ELIGIBLE, "spec_kind": _lib.ENERGY_GMM})
    for change in (dict(is_cuda=False), dict(dtype=torch.float64), dict(ndim=3), dict(dim=257), dict(spec_kind=None),
                   dict(spec_kind=_lib.ENERGY_MLP), dict(constant=False), dict(has_model_kwargs=True), dict(plain_integrator=False),
                   dict(autocast=True), dict(extras_ok=False)):
        assert not fused_moments_eligible(**{**ELIGIBLE, **change}), change


def test_cpu_calls_never_reach_the_entry():
    before = hip_calls(ENTRY)
    s = ta.LangevinDynamics(ta.DoubleWellModel(), step_size=0.01)
    s.sample_moments(x=torch.zeros(3, 2), n_steps=4)
    h = ta.HamiltonianMonteCarlo(ta.DoubleWellModel(), step_size=0.1, n_leapfrog_steps=2)
    h.sample_moments(x=torch.zeros(3, 2), n_steps=4)
    assert hip_calls(ENTRY) == before


@gpu
def test_sample_moments_is_one_launch_and_samples_states(cuda_device):
    dev, (n, dim, k) = cuda_device, (300, 6, 40)
    x0 = torch.randn(n, dim, device=dev)
    keep = x0.clone()
    s = ta.LangevinDynamics(ta.DoubleWellModel(device=dev), step_size=0.01, device=dev)
    g = torch.Generator(device=dev).manual_seed(5)
    before = hip_calls(ENTRY)
    x, mom = s.sample_moments(x=x0, n_steps=k, burn_in=6, energy=True, generator=g)
    assert hip_calls(ENTRY) == before + 1
    assert _rng._get_offset(g) == 4 * k
    assert torch.equal(x0, keep), "the caller's tensor was touched"
    want = s.sample(x=x0, n_steps=k, generator=torch.Generator(device=dev).manual_seed(5))
    assert torch.equal(x, want)
    assert mom.chain_mean.shape == (2, n, dim) and mom.chain_m2.shape == (2, n, dim) and mom.chain_mean.is_cuda
    assert mom.energy_mean.shape == (2, n) and mom.energy_m2.shape == (2, n) and mom.half_len == 17 and mom.acceptance_rate is None
    assert mom.n_nonfinite == 0 and torch.isfinite(mom.rhat).all() and torch.isfinite(mom.ess).all() and mom.rhat.shape == (dim,)
    assert torch.isfinite(mom.energy_rhat) and (mom.chain_m2 >= 0).all()
    _, plain = s.sample_moments(x=x0, n_steps=k, burn_in=6, generator=torch.Generator(device=dev).manual_seed(5))
    assert plain.energy_mean is None and torch.equal(plain.chain_mean, mom.chain_mean) and torch.equal(plain.chain_m2, mom.chain_m2)
    # HMC: one launch, 2 k Philox steps, the energy by default
    hm = ta.HamiltonianMonteCarlo(ta.core.ring_mixture(8, dim, device=dev), step_size=0.3, n_leapfrog_steps=3, device=dev)
    g = torch.Generator(device=dev).manual_seed(6)
    before = hip_calls(ENTRY)
    x, mom = hm.sample_moments(x=x0, n_steps=k, generator=g)
    assert hip_calls(ENTRY) == before + 1 and _rng._get_offset(g) == 4 * 2 * k
    assert mom.energy_mean is not None and mom.acceptance_rate.shape == (k,) and mom.half_len == 20
    assert ((mom.acceptance_rate > 0.3) & (mom.acceptance_rate <= 1.0)).all(), mom.acceptance_rate
    assert torch.isfinite(x).all() and mom.n_nonfinite == 0


@gpu
def test_other_configurations_take_the_eager_route_on_the_gpu(cuda_device):
    """A scheduled step size, a mass vector and an nn.Module energy: no call of the entry, and the law of the CPU eager route
    (pooled mean and variance of a harmonic well agree within the sampling error of 512 chains x 40 counted states)."""
    dev, (n, dim, k) = cuda_device, (512, 4, 60)

    class Quadratic(ta.BaseModel):
        def forward(self, x):
            return 2.0 * (x**2).sum(dim=-1)

    def configs(d):
        return {
            "scheduled": ta.LangevinDynamics(ta.HarmonicModel(k=4.0, device=d), step_size=ta.core.schedules.LinearScheduler(0.05, 0.04, 100),
                                             device=d),
            "mass": ta.HamiltonianMonteCarlo(ta.HarmonicModel(k=4.0, device=d), step_size=0.3, n_leapfrog_steps=3,
                                             mass=torch.full((dim,), 1.5, device=d), device=d),
            "module": ta.LangevinDynamics(Quadratic(device=d), step_size=0.05, device=d),
        }

    before = hip_calls(ENTRY)
    x0 = 0.5 * torch.randn(n, dim, generator=torch.Generator().manual_seed(2))
    on_gpu, on_cpu = configs(dev), configs(torch.device("cpu"))
    assert len(on_gpu) == 3
    for name in on_gpu:
        xg, mg = on_gpu[name].sample_moments(x=x0.to(dev), n_steps=k, burn_in=20, generator=torch.Generator(device=dev).manual_seed(1))
        xc, mc = on_cpu[name].sample_moments(x=x0, n_steps=k, burn_in=20, generator=torch.Generator().manual_seed(1))
        assert xg.is_cuda and mg.chain_mean.is_cuda and mg.n_nonfinite == 0 and mg.half_len == mc.half_len == 20
        # a harmonic well of variance about 1 / 4: 512 x 40 correlated states pin the pooled variance to a few per cent
        print(name, "var gpu", mg.var.tolist(), "cpu", mc.var.tolist())
        assert torch.allclose(mg.var.cpu(), mc.var, rtol=0.25) and (mg.mean.cpu() - mc.mean).abs().max() < 0.1
    assert hip_calls(ENTRY) == before


@gpu
def test_harmonic_chain_meets_the_closed_form_on_the_fused_route(cuda_device):
    from test_moments import check_harmonic_law, harmonic_closed_form

    dev, (n, h) = cuda_device, (4096, 200)
    v, _, _ = harmonic_closed_form(h)
    s = ta.LangevinDynamics(ta.HarmonicModel(k=4.0, device=dev), step_size=0.05, noise_scale=1.0, device=dev)
    x0 = (math.sqrt(v) * torch.randn(n, 4, generator=torch.Generator().manual_seed(0))).to(dev)
    before = hip_calls(ENTRY)
    _, mom = s.sample_moments(x=x0, n_steps=2 * h, generator=torch.Generator(device=dev).manual_seed(0))
    assert hip_calls(ENTRY) == before + 1
    check_harmonic_law(mom, n, h)
