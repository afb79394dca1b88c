"""ebm_ghmc_adapt_chain_mass_f32 on the GPU: every case of adapt_mass_cases.py against the restatement (decisions exactly, states
and step sizes by the fp64 yardstick), the three identities of the contract bit for bit (mass one is the unit-mass adapting entry,
the frozen run is the massed entry, two calls are one), native draws, sub-blocks, the optional outputs, what is written and what is
not, wild coordinates, the refusals, adapt_step_size with the opt-in and warmup() on top of it, and the law of the pooled step
size under a diagonal mass."""

import math

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib, _rng
from torchebm_amd.samplers import adapt
from helpers import hip_calls, to64, yardstick
import adapt_mass_cases as amc
import mass_cases as mc
from adapt_mass_cases import BOUNDS, CASES, DELTA, GAMMA, TEMP, case, energy_spec, ghmc_step, model_of, oracle_of, restate
from test_adapt_gpu import run_entry as run_unit
from test_mass_gpu import FILL, _field, _guarded, _mass_on, run_ghmc

gpu = pytest.mark.gpu
ENTRY = "ebm_ghmc_adapt_chain_mass_f32"
UNIT_ENTRY = "ebm_ghmc_adapt_chain_f32"
# The bar on the population median of an error against the fp64 restatement, in units of the fp32 restatement's own: the factor
# test_adapt_gpu.py and test_mass_gpu.py give this trajectory code.
K_MED = 2.0


def run_entry(dev, spec, mass, x0, p0, n_mh, thin, L, eps0, *, gamma=GAMMA, temp=TEMP, z=None, u=None, traj=True, mask=True,
              trace=True, alpha=True, n_adapt=None, m0=0, init_da=_lib.DA_INIT, da=None, mu=None, delta=DELTA, bounds=BOUNDS, seed=0,
              offset=0):
    """One call of the entry -> dict of CPU tensors x, v (the momentum) [n, dim], traj [n, n_mh // thin, dim], accepted [n_mh, n],
    da [3, n], eps_trace [n_mh, n], alpha_mean [n].  Outputs start from FILL and sit in front of a guard, as the mass does: a slot
    the call did not write keeps it, and so must the guards and the mass."""
    n, dim = x0.shape
    n_adapt = n_mh if n_adapt is None else n_adapt
    mu = math.log(amc.MU_FACTOR * eps0) if mu is None else mu
    model = model_of(spec, dev)
    x, gx = _guarded(dev, (n, dim), x0)
    v, gv = _guarded(dev, (n, dim), p0)
    d, gd = _guarded(dev, (3, n), da)
    tr, gt = _guarded(dev, (n, n_mh // thin, dim)) if traj else (None, None)
    mk, gk = _guarded(dev, (n_mh, n), dtype=torch.uint8) if mask else (None, None)
    et, ge = _guarded(dev, (n_mh, n)) if trace else (None, None)
    am, ga = _guarded(dev, (n,)) if alpha else (None, None)
    tab = amc.table(n_adapt, m0).to(dev)
    z_d = None if z is None else z.to(dev).contiguous()
    u_d = None if u is None else u.to(dev).contiguous()
    m_args, m_dev, gm = _mass_on(dev, mass, dim)
    before = hip_calls(ENTRY)
    _lib.call(ENTRY, model.fused_spec().to_c(), x.data_ptr(), v.data_ptr(), n, dim, n_mh, L, eps0, delta, mu, bounds[0], bounds[1], n_adapt,
              init_da, d.data_ptr(), _lib.ptr(tab) if n_adapt else None, _lib.ptr(et), _lib.ptr(am), gamma, temp, *m_args,
              int(p0 is None), thin, _lib.ptr(tr), _lib.ptr(mk), _lib.ptr(z_d), _lib.ptr(u_d), seed, offset, _lib.stream_handle(dev))
    torch.cuda.synchronize()
    assert hip_calls(ENTRY) == before + 1
    for guard in (gx, gv, gd, gt, gk, ge, ga, gm):
        assert guard is None or bool((guard == FILL).all()), "the call wrote behind a buffer"
    assert m_dev is None or torch.equal(m_dev.cpu(), mass), "the mass was written"
    cpu = lambda t: None if t is None else t.cpu()  # noqa: E731
    out = {"x": x.cpu(), "v": v.cpu(), "da": d.cpu(), "traj": cpu(tr), "eps_trace": cpu(et), "alpha_mean": cpu(am), "accepted": None}
    if mask:
        mk = mk.cpu()
        assert int(mk.max()) <= 1, "a row of the accept mask was not written"
        out["accepted"] = mk.bool()
    return out


def _run_case(dev, c, **kw):
    kw = {**dict(z=c["z"], u=c["u"]), **kw}
    return run_entry(dev, c["spec"], c["mass"], c["x0"], c["v0"], c["n_mh"], c["thin"], c["L"], c["eps0"], gamma=c["gamma"], temp=c["temp"],
                     **kw)


def _yard(got, ref32, ref64, what):
    """Print the ratio of the medians in front of the assertion (a missed bar leaves its figure in the output)."""
    err_ref = (ref32.double() - ref64).abs().amax(dim=1).median().item()
    err_hip = (got.double() - ref64).abs().amax(dim=1).median().item()
    print(f"{what}: median error {err_hip:.3e} against the fp32 restatement's {err_ref:.3e}, ratio {err_hip / max(err_ref, 1e-300):.3f}")
    return yardstick(got, ref32, ref64, k_med=K_MED, what=what)


# ---------------------------------------------------------------------------------
# 1. injected draws, every case
# ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind,dim,n,n_mh,thin,L,form", CASES)
def test_cases_with_injected_draws(cuda_device, kind, dim, n, n_mh, thin, L, form):
    c = case(kind, dim, n, n_mh, thin, L, form)
    ref32, ref64 = c["ref32"], c["ref64"]
    got = _run_case(cuda_device, c)
    assert torch.equal(got["accepted"], ref32["accepted"])
    assert got["traj"].shape == (n, n_mh // thin, dim) and not bool((got["traj"] == FILL).any())
    rows = lambda t: t.reshape(-1, dim)  # noqa: E731
    tag = f"{kind} dim {dim} {form} n_mh {n_mh}"
    _yard(got["x"], ref32["x"], ref64["x"], f"adapt_mass x {tag}")
    _yard(got["v"], ref32["v"], ref64["v"], f"adapt_mass p {tag}")
    _yard(rows(got["traj"]), rows(ref32["traj"]), rows(ref64["traj"]), f"adapt_mass traj {tag}")
    _yard(got["da"][0][:, None], ref32["da"][0][:, None], ref64["da"][0][:, None], f"adapt_mass step_sizes {tag}")
    _yard(got["eps_trace"].t(), ref32["eps_trace"].t(), ref64["eps_trace"].t(), f"adapt_mass eps_trace {tag}")
    assert torch.equal(got["eps_trace"][0], torch.full((n,), amc.f32(c["eps0"])))
    assert bool((got["alpha_mean"] >= 0).all()) and bool((got["alpha_mean"] <= 1).all())
    if n_mh % thin == 0:
        assert torch.equal(got["traj"][:, -1], got["x"])


# ---------------------------------------------------------------------------------
# 2. the identities of the contract
# ---------------------------------------------------------------------------------
IDENTITY_SHAPES = [("double_well", 5), ("double_well", 100), ("gmm", 32), ("gaussian", 100)]  # (5, 100: masked rows)


def _identity_inputs(kind, dim, n, n_mh, seed):
    g = torch.Generator().manual_seed(seed)
    x0 = mc.start_scale(kind) * torch.randn(n, dim, generator=g)
    v0 = torch.randn(n, dim, generator=g)
    return x0, v0, torch.randn(n_mh, n, dim, generator=g), torch.rand(n_mh, n, generator=g)


@gpu
@pytest.mark.parametrize("kind,dim", IDENTITY_SHAPES)
def test_mass_one_is_the_unit_mass_adapting_entry(cuda_device, kind, dim):
    """(a) mass_scalar = 1.0 or a diagonal of ones: x, v, da, traj, the mask, eps_trace and alpha_mean are
    ebm_ghmc_adapt_chain_f32's bit for bit, with injected and with native draws, with and without draw_v0."""
    dev, (n, n_mh, thin, L) = cuda_device, (111, 5, 2, 3)
    spec, eps0 = energy_spec(kind, dim), 2.0 * mc.ghmc_cases.step_size(kind, dim)
    x0, v0, z, u = _identity_inputs(kind, dim, n, n_mh, 21)
    seen = torch.zeros(2, dtype=torch.bool)
    for draws in (dict(z=z, u=u), dict(seed=0x1234567887654321, offset=77)):
        for start in (v0, None):
            want = run_unit(dev, spec, x0, start, n_mh, thin, L, eps0, **draws)
            for mass in (1.0, torch.ones(dim)):
                got = run_entry(dev, spec, mass, x0, start, n_mh, thin, L, eps0, **draws)
                for key in ("x", "v", "da", "traj", "accepted", "eps_trace", "alpha_mean"):
                    assert torch.equal(got[key], want[key]), (kind, dim, key, sorted(draws), type(mass).__name__)
            seen |= torch.tensor([bool(want["accepted"].any()), bool((~want["accepted"]).any())])
            assert not torch.equal(want["da"][0], torch.full((n,), amc.f32(eps0)))
    assert seen.all(), "the runs did not take both decisions"


@gpu
@pytest.mark.parametrize("form", ["scalar", "diag"])
@pytest.mark.parametrize("kind,dim", IDENTITY_SHAPES)
def test_the_frozen_run_is_the_massed_entry(cuda_device, kind, dim, form):
    """(b) n_adapt = 0, gamma = inf, da row 0 == eps: x, p, traj and the mask are ebm_ghmc_chain_mass_f32's at that eps and the
    same mass bit for bit -- a step size, a drift and a refresh held per lane leave the trajectory's arithmetic alone."""
    dev, (n, n_mh, thin, L) = cuda_device, (111, 5, 2, 3)
    spec, mass = energy_spec(kind, dim), mc.mass_of(form, dim)
    eps32 = amc.f32(2.0 * ghmc_step(kind, dim, mass))
    x0, v0, z, u = _identity_inputs(kind, dim, n, n_mh, 22)
    p0 = mc.forms(mass, torch.float32)[1] * v0
    da = torch.stack((torch.full((n,), eps32), torch.full((n,), 0.25), torch.full((n,), -0.5)))
    seen = torch.zeros(2, dtype=torch.bool)
    for temp in (1.0, TEMP):
        for draws in (dict(z=z, u=u), dict(seed=0x1234567887654321, offset=77)):
            for start in (p0, None):
                want = run_ghmc(dev, spec, mass, x0, start, n_mh, thin, L, eps32, gamma=math.inf, temp=temp, **draws)
                got = run_entry(dev, spec, mass, x0, start, n_mh, thin, L, 0.5 * eps32, gamma=math.inf, temp=temp, n_adapt=0, init_da=0,
                                da=da, **draws)
                for key in ("x", "v", "traj", "accepted"):
                    assert torch.equal(got[key], want[key]), (kind, dim, form, temp, key, sorted(draws))
                assert torch.equal(got["da"], da) and torch.equal(got["eps_trace"], torch.full((n_mh, n), eps32))
                assert torch.equal(got["alpha_mean"], torch.zeros(n))
                seen |= torch.tensor([bool(want["accepted"].any()), bool((~want["accepted"]).any())])
    assert seen.all(), "the runs did not take both decisions"


@gpu
@pytest.mark.parametrize("dim", [5, 100])
def test_the_frozen_run_at_unit_temperature_is_the_hmc_kernels(cuda_device, dim):
    """(b) with T = 1: ebm_hmc_chain_f32's x and mask with the same diagonal mass."""
    dev, (n, n_mh, L) = cuda_device, (111, 5, 4)
    spec, mass = energy_spec("double_well", dim), mc.diag_mass(dim)
    eps32 = amc.f32(0.15 * math.sqrt(mc.min_mass(mass)))
    x0, v0, z, u = _identity_inputs("double_well", dim, n, n_mh, 23)
    da = torch.stack((torch.full((n,), eps32), torch.zeros(n), torch.zeros(n)))
    got = run_entry(dev, spec, mass, x0, v0, n_mh, 1, L, 1.0, gamma=math.inf, temp=1.0, n_adapt=0, init_da=0, da=da, z=z, u=u)
    rows, p_d, u_d, m_d = x0.to(dev).clone(), z.to(dev), u.to(dev), mass.to(dev)
    mask = torch.empty(n_mh, n, dtype=torch.uint8, device=dev)
    _lib.call("ebm_hmc_chain_f32", model_of(spec, dev).fused_spec().to_c(), rows.data_ptr(), n, dim, n_mh, L, eps32, None, _lib.MASS_DIAG,
              0.0, m_d.data_ptr(), 1, None, None, mask.data_ptr(), None, p_d.data_ptr(), u_d.data_ptr(), 0, 0, _lib.stream_handle(dev))
    torch.cuda.synchronize()
    assert torch.equal(mask.cpu().bool(), got["accepted"]) and (~got["accepted"]).any() and got["accepted"].any()
    assert torch.equal(rows.cpu(), got["x"])


@gpu
@pytest.mark.parametrize("form", ["scalar", "diag"])
@pytest.mark.parametrize("kind,dim", IDENTITY_SHAPES)
def test_two_calls_are_one(cuda_device, kind, dim, form):
    """(c) n_adapt == n_mh in both calls: (n1, m0 = 0, open) then (n2, m0 = n1, init_da = 0) is one call of n1 + n2, da included;
    and a closed call followed by a frozen one is one call whose adaptation ends at n1.  Native and injected draws; the first call
    draws its momenta or is handed them."""
    dev, (n, n1, n2, L) = cuda_device, (37, 4, 7, 3)
    spec, mass = energy_spec(kind, dim), mc.mass_of(form, dim)
    eps0 = ghmc_step(kind, dim, mass)
    x0, v0, z, u = _identity_inputs(kind, dim, n, n1 + n2, 6)
    p0 = mc.forms(mass, torch.float32)[1] * v0
    seed, offset = 0x0123456789ABCDEF, 41
    kw = dict(mu=math.log(10.0 * eps0))
    for injected in (False, True):
        for start in (None, p0):
            if injected:
                all_, a_, b_ = dict(z=z, u=u, seed=seed, offset=offset), dict(z=z[:n1], u=u[:n1], seed=seed, offset=offset), dict(z=z[n1:], u=u[n1:])
            else:
                all_, a_, b_ = dict(seed=seed, offset=offset), dict(seed=seed, offset=offset), dict(seed=seed, offset=offset + 2 * n1)
            run = lambda x, p, k, **more: run_entry(dev, spec, mass, x, p, k, 1, L, eps0, **kw, **more)  # noqa: E731
            whole = run(x0, start, n1 + n2, **all_)
            first = run(x0, start, n1, init_da=_lib.DA_INIT | _lib.DA_OPEN, **a_)
            second = run(first["x"], first["v"], n2, init_da=0, da=first["da"], m0=n1, **b_)
            for key in ("x", "v", "da"):
                assert torch.equal(second[key], whole[key]), (key, injected)
            for key in ("traj", "accepted", "eps_trace"):
                assert torch.equal(torch.cat((first[key], second[key]), dim=1 if key == "traj" else 0), whole[key]), (key, injected)
            assert not torch.equal(whole["da"][0], torch.full((n,), amc.f32(eps0)))
            whole = run(x0, start, n1 + n2, n_adapt=n1, **all_)
            first = run(x0, start, n1, **a_)
            second = run(first["x"], first["v"], n2, init_da=0, da=first["da"], n_adapt=0, **b_)
            for key in ("x", "v", "da"):
                assert torch.equal(second[key], whole[key]), (key, injected)
            assert torch.equal(torch.cat((first["eps_trace"], second["eps_trace"])), whole["eps_trace"])
            assert torch.equal(second["da"], first["da"]) and torch.equal(whole["eps_trace"][-1], whole["da"][0])


# ---------------------------------------------------------------------------------
# 3. native draws, sub-blocks
# ---------------------------------------------------------------------------------
def _fields(dev, mass, seed, offset, n, dim, n_mh, temp):
    """p0, z, u of a call at (seed, offset): step `offset` scaled by sqrt_temp m_sqrt, normals at offset + 1 + 2 t, uniforms at
    offset + 2 + 2 t."""
    z0 = _field(dev, _lib.NOISE_NORMAL, seed, offset, n * dim).view(n, dim).cpu()
    p0 = (amc.f32(math.sqrt(temp)) * mc.forms(mass, torch.float32)[1]) * z0
    z = torch.stack([_field(dev, _lib.NOISE_NORMAL, seed, offset + 1 + 2 * t, n * dim) for t in range(n_mh)]).view(n_mh, n, dim).cpu()
    u = torch.stack([_field(dev, _lib.NOISE_UNIFORM, seed, offset + 2 + 2 * t, n) for t in range(n_mh)]).view(n_mh, n).cpu()
    return p0, z, u


@gpu
def test_native_draws_are_the_materialised_fields(cuda_device):
    dev, (n_mh, thin) = cuda_device, (7, 3)
    rejected = 0
    for kind, dim, n, form in [("double_well", 5, 37, "diag"), ("harmonic", 100, 37, "scalar"), ("gmm", 32, 70, "diag"),
                               ("gaussian", 256, 9, "diag")]:
        spec, mass, L = energy_spec(kind, dim), mc.mass_of(form, dim), 2
        eps0 = ghmc_step(kind, dim, mass)
        x0 = mc.start_scale(kind) * torch.randn(n, dim, generator=torch.Generator().manual_seed(5))
        seed, offset = 0x1234567887654321, 77
        p0, z, u = _fields(dev, mass, seed, offset, n, dim, n_mh, TEMP)
        native = run_entry(dev, spec, mass, x0, None, n_mh, thin, L, eps0, seed=seed, offset=offset)
        fed = run_entry(dev, spec, mass, x0, p0, n_mh, thin, L, eps0, z=z, u=u)
        for key in ("x", "v", "traj", "accepted", "da", "eps_trace", "alpha_mean"):
            assert torch.equal(native[key], fed[key]), (kind, key)
            assert torch.isfinite(native[key].float()).all()
        rejected += int((~native["accepted"]).sum())
        # a sub-block of chains run alone (another grid, other lanes) reproduces its rows of the full launch
        lo, hi = n // 3, n // 3 + max(n // 2, 1)
        part = run_entry(dev, spec, mass, x0[lo:hi], p0[lo:hi], n_mh, thin, L, eps0, z=z[:, lo:hi], u=u[:, lo:hi])
        for key in ("x", "v", "traj", "alpha_mean"):
            assert torch.equal(part[key], fed[key][lo:hi]), (kind, key)
        for key in ("accepted", "da", "eps_trace"):
            assert torch.equal(part[key], fed[key][:, lo:hi]), (kind, key)
    assert rejected > 0, "no proposal was rejected: the accept uniforms were not exercised"


# ---------------------------------------------------------------------------------
# 4. optional outputs, written rows and guards
# ---------------------------------------------------------------------------------
def _cases_of(kind, form, n_mh=4):
    return [c for c in CASES if c[0] == kind and c[6] == form and c[3] == n_mh]


@gpu
@pytest.mark.parametrize("kind,dim,n,n_mh,thin,L,form", [_cases_of("double_well", "diag")[0], _cases_of("harmonic", "scalar")[0],
                                                        _cases_of("gaussian", "diag")[-1], _cases_of("rosenbrock", "diag")[0]])
def test_every_row_is_written_and_each_output_is_optional(cuda_device, kind, dim, n, n_mh, thin, L, form):
    c = case(kind, dim, n, n_mh, thin, L, form)
    got = _run_case(cuda_device, c)  # (run_entry checks the guard behind every buffer, the mass, and that every mask row is 0 / 1)
    for key in ("x", "v", "traj", "da", "eps_trace", "alpha_mean"):
        assert not bool((got[key] == FILL).any()), f"a slot of {key} was not written"
    names = {"traj": "traj", "mask": "accepted", "trace": "eps_trace", "alpha": "alpha_mean"}
    for off in list(names) + [None]:  # each alone, then all four
        kw = {name: False for name in (names if off is None else [off])}
        lean = _run_case(cuda_device, c, **kw)
        for name, key in names.items():
            if name in kw:
                assert lean[key] is None
            else:
                assert torch.equal(lean[key], got[key]), (off, key)
        for key in ("x", "v", "da"):
            assert torch.equal(lean[key], got[key]), (off, key)
    # draw_v0: the momentum plane is output only; init_da: da is output only -- every row written
    drawn = run_entry(cuda_device, c["spec"], c["mass"], c["x0"], None, n_mh, thin, L, c["eps0"], z=c["z"], u=c["u"], seed=3, offset=9)
    assert not bool((drawn["v"] == FILL).any()) and torch.isfinite(drawn["v"]).all() and not bool((drawn["da"] == FILL).any())


# ---------------------------------------------------------------------------------
# 5. wild coordinates
# ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind,dim,n,n_mh,thin,L,form", [_cases_of("double_well", "diag")[0], _cases_of("gaussian", "scalar")[0]])
def test_wild_start_stays_in_its_chain(cuda_device, kind, dim, n, n_mh, thin, L, form):
    """A NaN coordinate in one chain and a 1e20 coordinate in another: every other chain's outputs, decisions and step sizes are
    bitwise the clean run's, and the wild chains' step sizes stay inside the bounds.  (The bounds hold up to the rounding of their
    logs to fp32, |log b| 2^-24 <= 4e-7 here, and of expf, 2 ulp: 1e-6 relative covers both.)"""
    c = case(kind, dim, n, n_mh, thin, L, form)
    bounds = (0.25 * c["eps0"], 4.0 * c["eps0"])
    x0 = c["x0"].clone()
    x0[3, 2] = float("nan")
    x0[7, 4] = 1e20
    got = run_entry(cuda_device, c["spec"], c["mass"], x0, c["v0"], n_mh, thin, L, c["eps0"], z=c["z"], u=c["u"], bounds=bounds)
    clean = _run_case(cuda_device, c, bounds=bounds)
    others = [i for i in range(n) if i not in (3, 7)]
    for key in ("x", "v", "traj", "alpha_mean"):
        assert torch.isfinite(clean[key]).all()
        assert torch.equal(got[key][others], clean[key][others]), key
    for key in ("accepted", "da", "eps_trace"):
        assert torch.equal(got[key][:, others], clean[key][:, others]), key
    assert torch.isnan(got["x"][3]).any() and not got["accepted"][:, 3].any()  # the NaN chain held its state and only flipped
    for eps in (got["eps_trace"], got["da"][0]):
        assert torch.isfinite(eps).all() and bool((eps >= bounds[0] * (1 - 1e-6)).all()) and bool((eps <= bounds[1] * (1 + 1e-6)).all())
    assert got["alpha_mean"][3] == 0 and math.isclose(got["eps_trace"][-1, 3].item(), bounds[0], rel_tol=1e-6)
    assert torch.isfinite(got["da"]).all()


# ---------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------
@gpu
def test_refusals_launch_nothing(cuda_device):
    """The refusals of test_adapt_mass.py with real buffers: each raises its code and no buffer is touched."""
    from test_adapt_mass import REFUSALS, _abi_call

    dev, (n, dim) = cuda_device, (4, 8)
    bufs = {name: torch.full((n, 260), FILL, device=dev) for name in ("x", "v", "da", "table", "trace", "alpha", "traj", "mass_diag")}
    bufs["mask"] = torch.full((n, 260), 7, device=dev, dtype=torch.uint8)
    real = {name: t.data_ptr() for name, t in bufs.items()}
    desc = model_of(energy_spec("double_well", dim), dev).fused_spec().to_c()
    for kw, exc, match in REFUSALS:
        with pytest.raises(exc, match=match):
            _abi_call(desc, **{**real, **kw})
    mlp = ta.MLPEnergy(dim, 64, device=dev)
    with pytest.raises(RuntimeError, match=r"code -2"):
        _abi_call(mlp.fused_spec().to_c(), **real)
    torch.cuda.synchronize()
    for t in bufs.values():
        assert bool((t == 7).all())


# ---------------------------------------------------------------------------------
# 7. through adapt_step_size and warmup
# ---------------------------------------------------------------------------------
def _sampler(which, spec, dev, eps0, L, mass):
    if which == "ghmc":
        return ta.GeneralizedHMC(model_of(spec, dev), step_size=eps0, n_leapfrog_steps=L, friction=GAMMA, temperature=TEMP, device=dev,
                                 mass=mass), GAMMA, TEMP
    return ta.HamiltonianMonteCarlo(model_of(spec, dev), step_size=eps0, n_leapfrog_steps=L, device=dev, mass=mass), math.inf, 1.0


@gpu
@pytest.mark.parametrize("form", ["scalar", "diag"])
@pytest.mark.parametrize("which", ["ghmc", "hmc"])
def test_adapt_step_size_with_the_opt_in_is_one_launch(cuda_device, which, form):
    dev, (n, dim, k, L) = cuda_device, (300, 6, 40, 3)
    spec, mass = energy_spec("double_well", dim), mc.mass_of(form, dim)
    eps0 = 0.02 * math.sqrt(mc.min_mass(mass))
    s, gamma, temp = _sampler(which, spec, dev, eps0, L, mass if form == "scalar" else mass.to(dev))
    x0 = torch.randn(n, dim, device=dev)
    keep = x0.clone()
    assert adapt.adapt_route(s, x0, gamma)[0] == "eager"  # off, the default
    s.fused_adapt_mass = True
    assert adapt.adapt_route(s, x0, gamma)[0] == "fused_mass"
    g = torch.Generator(device=dev).manual_seed(5)
    before = dict(_lib.call_counts)
    r = s.adapt_step_size(x=x0, n_steps=k, generator=g, apply=False)
    torch.cuda.synchronize()
    new = {name: c - before.get(name, 0) for name, c in _lib.call_counts.items() if c != before.get(name, 0)}
    assert new == {ENTRY: 1}, new
    assert _rng._get_offset(g) == 4 * (2 * k + 1)
    assert torch.equal(x0, keep), "the caller's tensor was touched"
    assert s.get_scheduled_value("step_size") == eps0
    if form == "diag":
        assert torch.equal(s.mass.cpu(), mass), "the sampler's mass was touched"
    # the result is the entry's at the generator's coordinates
    want = run_entry(dev, spec, mass, x0.cpu(), None, k, 1, L, eps0, gamma=gamma, temp=temp, seed=_rng.kernel_seed(5), offset=0)
    assert torch.equal(r.x.cpu(), want["x"]) and torch.equal(r.velocity.cpu(), want["v"]) and torch.equal(r.da.cpu(), want["da"])
    assert torch.equal(r.step_sizes.cpu(), want["da"][0]) and torch.equal(r.acceptance.cpu(), want["alpha_mean"])
    assert r.step_size.ndim == 0 and r.step_size.is_cuda and torch.allclose(r.step_size.cpu(), want["da"][0].log().median().exp(), rtol=1e-6)
    assert want["accepted"].any() and (~want["accepted"]).any() and float(r.step_size) > 2.0 * eps0
    # apply, with a passed momentum plane that stays untouched
    p0 = torch.randn(n, dim, device=dev)
    p_keep = p0.clone()
    r = s.adapt_step_size(x=x0, n_steps=k, velocity=p0, generator=g)
    assert torch.equal(p0, p_keep) and s.get_scheduled_value("step_size") == float(r.step_size)


@gpu
def test_without_the_opt_in_and_outside_the_conditions_the_route_is_eager(cuda_device):
    dev, (n, k, L) = cuda_device, (64, 8, 2)
    before = hip_calls(ENTRY)
    sched = lambda: ta.core.schedules.LinearScheduler(0.3, 0.1, 10)  # noqa: E731
    for cls in (ta.GeneralizedHMC, ta.HamiltonianMonteCarlo):
        for dim, opt_in, kw in ((4, False, dict(step_size=0.1)), (4, True, dict(step_size=sched())), (300, True, dict(step_size=0.1))):
            s = cls(ta.HarmonicModel(k=4.0, device=dev), n_leapfrog_steps=L, device=dev, mass=2.0, **kw)
            s.fused_adapt_mass = opt_in
            x0 = 0.5 * torch.randn(n, dim, device=dev)
            assert adapt.adapt_route(s, x0, 1.0)[0] == "eager"
            r = s.adapt_step_size(x=x0, n_steps=k, generator=torch.Generator(device=dev).manual_seed(2))
            assert r.x.is_cuda and r.x.shape == (n, dim) and torch.isfinite(r.step_sizes).all() and float(r.step_size) > 0
    assert hip_calls(ENTRY) == before


@gpu
@pytest.mark.parametrize("which", ["ghmc", "hmc"])
def test_warmup_is_one_launch_per_window(cuda_device, which):
    """len(windows) + 1 launches of chain entries -- the unit-mass adapting entry while the mass is None, the massed one from then
    on -- and nothing else through the library; the result is the composition written out with public calls under the opt-in."""
    dev, (n, dim, L, eps0) = cuda_device, (512, 6, 3, 0.02)
    spec = energy_spec("double_well", dim)
    windows, final = (6, 5, 7), 4
    s, _, _ = _sampler(which, spec, dev, eps0, L, None)
    x0 = torch.randn(n, dim, device=dev)
    keep = x0.clone()
    g = torch.Generator(device=dev).manual_seed(9)
    before = dict(_lib.call_counts)
    w = s.warmup(x=x0, windows=windows, final_steps=final, generator=g, apply=False)
    torch.cuda.synchronize()
    new = {name: c - before.get(name, 0) for name, c in _lib.call_counts.items() if c != before.get(name, 0)}
    assert new == {UNIT_ENTRY: 1, ENTRY: len(windows)}, new
    assert _rng._get_offset(g) == 4 * sum(2 * k + 1 for k in windows + (final,))
    assert torch.equal(x0, keep) and s.mass is None and s.get_scheduled_value("step_size") == eps0 and "fused_adapt_mass" not in vars(s)
    assert w.x.is_cuda and w.mass.is_cuda and w.mass.shape == (dim,) and len(w.step_sizes) == 4 and len(w.masses) == 3
    # written out
    s2, _, _ = _sampler(which, spec, dev, eps0, L, None)
    s2.fused_adapt_mass = True
    g2 = torch.Generator(device=dev).manual_seed(9)
    x, eps, prev = x0, None, torch.ones(dim, device=dev)
    for i, k in enumerate(windows + (final,)):
        r = s2.adapt_step_size(x=x, n_steps=k, velocity=None, init_step_size=eps, generator=g2, apply=False)
        x, eps = r.x, float(r.step_size)
        assert torch.equal(w.step_sizes[i], r.step_size) and torch.equal(w.acceptances[i], r.acceptance.mean())
        if i < len(windows):
            var = n / (n + 5.0) * x.var(0) + 1e-3 * (5.0 / (n + 5.0))
            prev = torch.where(torch.isfinite(var) & (var > 0), 1.0 / var, prev)
            s2.mass = prev
            assert torch.equal(w.masses[i], prev)
    assert torch.equal(w.x, x) and torch.equal(w.mass, prev) and float(w.step_size) == eps
    # a sampler that starts from a scalar mass: every window is the massed entry
    s3, _, _ = _sampler(which, spec, dev, eps0, L, 0.37)
    before = dict(_lib.call_counts)
    w = s3.warmup(x=x0, windows=(5,), final_steps=4, generator=g)
    new = {name: c - before.get(name, 0) for name, c in _lib.call_counts.items() if c != before.get(name, 0)}
    assert new == {ENTRY: 2}, new
    assert torch.equal(s3.mass, w.mass) and s3.get_scheduled_value("step_size") == float(w.step_size)


# ---------------------------------------------------------------------------------
# 8. the law
# ---------------------------------------------------------------------------------
@gpu
def test_the_pooled_step_size_is_the_restatements(cuda_device):
    """energy_spec("harmonic", 4) with a diagonal mass, a full refresh, L = 4, delta = 0.8, 4096 chains, 200 transitions: log
    step_size of the fused route (native draws) lies within 4.5 sqrt(se1^2 + se2^2) of the fp64 restatement's on torch draws,
    se = 1.2533 std(log eps-bar) / sqrt(n), each side's own -- test_adapt_gpu.py's bar."""
    dev, law = cuda_device, amc.LAW
    n, dim, k, L = law["n"], law["dim"], law["n_mh"], law["L"]
    spec, mass = energy_spec(law["kind"], dim), mc.diag_mass(dim)
    g = torch.Generator().manual_seed(0)
    x0 = torch.randn(n, dim, generator=g)
    z, u = torch.randn(k, n, dim, generator=g), torch.rand(k, n, generator=g)
    ref = restate(to64(oracle_of(spec)), x0, torch.zeros(n, dim), z, u, law["eps0"], L, math.inf, 1.0, mass, torch.float64, delta=law["delta"])
    s = ta.HamiltonianMonteCarlo(model_of(spec, dev), step_size=law["eps0"], n_leapfrog_steps=L, device=dev, mass=mass.to(dev))
    s.fused_adapt_mass = True
    before = hip_calls(ENTRY)
    r = s.adapt_step_size(x=x0.to(dev), n_steps=k, target_accept=law["delta"], generator=torch.Generator(device=dev).manual_seed(1))
    assert hip_calls(ENTRY) == before + 1
    got, se_got = amc.pooled_log(r.step_sizes.cpu())
    want, se_want = amc.pooled_log(ref["da"][0])
    bar = amc.LAW_SIGMAS * math.sqrt(se_got**2 + se_want**2)
    print(f"log step_size: fused {got:.5f} (se {se_got:.5f}), fp64 restatement {want:.5f} (se {se_want:.5f}), bar {bar:.5f}; "
          f"step sizes {math.exp(got):.4f} / {math.exp(want):.4f}; acceptance while adapting {r.acceptance.mean().item():.3f}")
    assert math.isclose(math.log(float(r.step_size)), got, abs_tol=1e-6)
    assert abs(got - want) < bar
    assert 0.7 < r.acceptance.mean().item() < 0.9
