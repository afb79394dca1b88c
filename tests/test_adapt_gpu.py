"""ebm_ghmc_adapt_chain_f32 on the GPU: every case of adapt_cases.py against the restatement (decisions exactly, states and step
sizes by the fp64 yardstick), the frozen run against ebm_ghmc_chain_f32 bit for bit, continuation, native draws, sub-blocks,
the optional outputs, what is written and what is not, wild coordinates, the refusals, adapt_step_size on top of it, and the law
of the pooled step size."""

import math

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib, _rng
from torchebm_amd.samplers import adapt
from helpers import hip_calls, to64, yardstick
import adapt_cases as ac
from adapt_cases import ALL_CASES, BOUNDS, CASES, DELTA, GAMMA, TEMP, case, energy_spec, model_of, oracle_of, restate, step_size
from test_ghmc_gpu import FILL, _field, _guarded
from test_ghmc_gpu import run_entry as run_plain

gpu = pytest.mark.gpu
ENTRY = "ebm_ghmc_adapt_chain_f32"
# The bar on the population median of an error against the fp64 restatement, in units of the fp32 restatement's own: the factor
# test_ghmc_gpu.py gives this trajectory code.
K_MED = 2.0


def run_entry(dev, spec, x0, v0, n_mh, thin, L, eps0, *, gamma=GAMMA, temp=TEMP, z=None, u=None, traj=True, mask=True, trace=True,
              alpha=True, n_adapt=None, m0=0, init_da=_lib.DA_INIT, da=None, mu=None, delta=DELTA, bounds=BOUNDS, seed=0, offset=0):
    """One call of the entry -> dict of CPU tensors x, v [n, dim], traj [n, n_mh // thin, dim], accepted [n_mh, n], da [3, n],
    eps_trace [n_mh, n], alpha_mean [n].  Outputs start from FILL and sit in front of a guard: a slot the call did not write
    keeps it, and so must the guards."""
    n, dim = x0.shape
    n_adapt = n_mh if n_adapt is None else n_adapt
    mu = math.log(ac.MU_FACTOR * eps0) if mu is None else mu
    model = model_of(spec, dev)
    x, gx = _guarded(dev, (n, dim), x0)
    v, gv = _guarded(dev, (n, dim), v0)
    d, gd = _guarded(dev, (3, n), da)
    tr, gt = _guarded(dev, (n, n_mh // thin, dim)) if traj else (None, None)
    mk, gm = _guarded(dev, (n_mh, n), dtype=torch.uint8) if mask else (None, None)
    et, ge = _guarded(dev, (n_mh, n)) if trace else (None, None)
    am, ga = _guarded(dev, (n,)) if alpha else (None, None)
    tab = ac.table(n_adapt, m0).to(dev)
    z_d = None if z is None else z.to(dev).contiguous()
    u_d = None if u is None else u.to(dev).contiguous()
    before = hip_calls(ENTRY)
    _lib.call(ENTRY, model.fused_spec().to_c(), x.data_ptr(), v.data_ptr(), n, dim, n_mh, L, eps0, delta, mu, bounds[0], bounds[1], n_adapt,
              init_da, d.data_ptr(), _lib.ptr(tab) if n_adapt else None, _lib.ptr(et), _lib.ptr(am), gamma, temp, int(v0 is None), thin,
              _lib.ptr(tr), _lib.ptr(mk), _lib.ptr(z_d), _lib.ptr(u_d), seed, offset, _lib.stream_handle(dev))
    torch.cuda.synchronize()
    assert hip_calls(ENTRY) == before + 1
    for guard in (gx, gv, gd, gt, gm, ge, ga):
        assert guard is None or bool((guard == FILL).all()), "the call wrote behind an output"
    cpu = lambda t: None if t is None else t.cpu()  # noqa: E731
    out = {"x": x.cpu(), "v": v.cpu(), "da": d.cpu(), "traj": cpu(tr), "eps_trace": cpu(et), "alpha_mean": cpu(am), "accepted": None}
    if mask:
        mk = mk.cpu()
        assert int(mk.max()) <= 1, "a row of the accept mask was not written"
        out["accepted"] = mk.bool()
    return out


def _run_case(dev, c, **kw):
    kw = {**dict(z=c["z"], u=c["u"]), **kw}
    return run_entry(dev, c["spec"], c["x0"], c["v0"], c["n_mh"], c["thin"], c["L"], c["eps0"], gamma=c["gamma"], temp=c["temp"], **kw)


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
@pytest.mark.parametrize("kind,dim,n,n_mh,thin,L", ALL_CASES)
def test_cases_with_injected_draws(cuda_device, kind, dim, n, n_mh, thin, L):
    c = case(kind, dim, n, n_mh, thin, L)
    ref32, ref64 = c["ref32"], c["ref64"]
    got = _run_case(cuda_device, c)
    assert torch.equal(got["accepted"], ref32["accepted"])
    assert got["traj"].shape == (n, n_mh // thin, dim) and not bool((got["traj"] == FILL).any())
    rows = lambda t: t.reshape(-1, dim)  # noqa: E731
    tag = f"{kind} dim {dim}"
    _yard(got["x"], ref32["x"], ref64["x"], f"adapt x {tag}")
    _yard(got["v"], ref32["v"], ref64["v"], f"adapt v {tag}")
    _yard(rows(got["traj"]), rows(ref32["traj"]), rows(ref64["traj"]), f"adapt traj {tag}")
    _yard(got["da"][0][:, None], ref32["da"][0][:, None], ref64["da"][0][:, None], f"adapt step_sizes {tag}")
    _yard(got["eps_trace"].t(), ref32["eps_trace"].t(), ref64["eps_trace"].t(), f"adapt eps_trace {tag}")
    # the step size a transition ran at is the one the transition before left, and the first is fp32(eps0)
    assert torch.equal(got["eps_trace"][0], torch.full((n,), ac.f32(c["eps0"])))
    # alpha_mean is a function of the same H0 - H1 the decisions above come from; its figure is printed, and its bits are held by
    # the continuation, sub-block, optional-output and wild-start tests below
    err_ref = (ref32["alpha_mean"].double() - ref64["alpha_mean"]).abs().mean().item()
    err_hip = (got["alpha_mean"].double() - ref64["alpha_mean"]).abs().mean().item()
    print(f"adapt alpha_mean {tag}: mean error {err_hip:.3e} against the fp32 restatement's {err_ref:.3e}")
    assert bool((got["alpha_mean"] >= 0).all()) and bool((got["alpha_mean"] <= 1).all())
    if n_mh % thin == 0:
        assert torch.equal(got["traj"][:, -1], got["x"])


# ---------------------------------------------------------------------------------
# 2. the frozen run is the plain entry
# ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", ["double_well", "gmm"])
@pytest.mark.parametrize("dim", [5, 100])
def test_the_frozen_run_is_the_plain_entry(cuda_device, kind, dim):
    """n_adapt = 0, gamma = inf, T = 1, da row 0 == eps: x, v, traj and the mask are ebm_ghmc_chain_f32's at that eps bit for bit --
    a step size held per lane leaves the trajectory's arithmetic alone."""
    dev, (n, n_mh, thin, L) = cuda_device, (111, 5, 2, 3)
    spec, eps = energy_spec(kind, dim), 2.0 * step_size(kind, dim)
    eps32 = ac.f32(eps)
    g = torch.Generator().manual_seed(21)
    x0, v0 = torch.randn(n, dim, generator=g), torch.randn(n, dim, generator=g)
    z, u = torch.randn(n_mh, n, dim, generator=g), torch.rand(n_mh, n, generator=g)
    da = torch.stack((torch.full((n,), eps32), torch.full((n,), 0.25), torch.full((n,), -0.5)))
    seen = torch.zeros(2, dtype=torch.bool)
    for draws in (dict(z=z, u=u), dict(seed=0x1234567887654321, offset=77)):
        for start in (v0, None):
            want = run_plain(dev, spec, x0, start, n_mh, thin, L, eps32, gamma=math.inf, temp=1.0, **draws)
            got = run_entry(dev, spec, x0, start, n_mh, thin, L, 0.5 * eps, gamma=math.inf, temp=1.0, n_adapt=0, init_da=0, da=da, **draws)
            for key in ("x", "v", "traj", "accepted"):
                assert torch.equal(got[key], want[key]), (kind, dim, key, sorted(draws))
            assert torch.equal(got["da"], da) and torch.equal(got["eps_trace"], torch.full((n_mh, n), eps32))
            assert torch.equal(got["alpha_mean"], torch.zeros(n))
            seen |= torch.tensor([bool(want["accepted"].any()), bool((~want["accepted"]).any())])
    assert seen.all(), "the runs did not take both decisions"


# ---------------------------------------------------------------------------------
# 3. continuation, native draws, sub-blocks
# ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind,dim", [("double_well", 5), ("gmm", 32), ("double_well", 100)])
def test_two_calls_are_one(cuda_device, kind, dim):
    """n_adapt == n_mh in both calls: (n1, m0 = 0, open) then (n2, m0 = n1, init_da = 0) is one call of n1 + n2, da included;
    and a closed call followed by a frozen one is one call whose adaptation ends at n1."""
    dev, (n, n1, n2, L) = cuda_device, (37, 4, 7, 3)
    spec, eps0 = energy_spec(kind, dim), step_size(kind, dim)
    x0 = torch.randn(n, dim, generator=torch.Generator().manual_seed(6))
    seed, offset = 0x0123456789ABCDEF, 41
    kw = dict(mu=math.log(10.0 * eps0), seed=seed)
    whole = run_entry(dev, spec, x0, None, n1 + n2, 1, L, eps0, offset=offset, **kw)
    first = run_entry(dev, spec, x0, None, n1, 1, L, eps0, offset=offset, init_da=_lib.DA_INIT | _lib.DA_OPEN, **kw)
    second = run_entry(dev, spec, first["x"], first["v"], n2, 1, L, eps0, offset=offset + 2 * n1, init_da=0, da=first["da"], m0=n1, **kw)
    for key in ("x", "v", "da"):
        assert torch.equal(second[key], whole[key]), key
    for key in ("traj", "accepted", "eps_trace"):
        assert torch.equal(torch.cat((first[key], second[key]), dim=1 if key == "traj" else 0), whole[key]), key
    assert not torch.equal(whole["da"][0], torch.full((n,), ac.f32(eps0))) and (~whole["accepted"]).any()
    whole = run_entry(dev, spec, x0, None, n1 + n2, 1, L, eps0, offset=offset, n_adapt=n1, **kw)
    first = run_entry(dev, spec, x0, None, n1, 1, L, eps0, offset=offset, **kw)
    second = run_entry(dev, spec, first["x"], first["v"], n2, 1, L, eps0, offset=offset + 2 * n1, init_da=0, da=first["da"], n_adapt=0, **kw)
    for key in ("x", "v", "da"):
        assert torch.equal(second[key], whole[key]), key
    assert torch.equal(torch.cat((first["eps_trace"], second["eps_trace"])), whole["eps_trace"])
    assert torch.equal(second["da"], first["da"]) and torch.equal(whole["eps_trace"][-1], whole["da"][0])


def _fields(dev, seed, offset, n, dim, n_mh, temp):
    """v0, z, u of a call at (seed, offset): step `offset` scaled by sqrt_temp, normals at offset + 1 + 2 t, uniforms at
    offset + 2 + 2 t."""
    v0 = (ac.f32(math.sqrt(temp)) * _field(dev, _lib.NOISE_NORMAL, seed, offset, n * dim)).view(n, dim).cpu()
    z = torch.stack([_field(dev, _lib.NOISE_NORMAL, seed, offset + 1 + 2 * t, n * dim) for t in range(n_mh)]).view(n_mh, n, dim).cpu()
    u = torch.stack([_field(dev, _lib.NOISE_UNIFORM, seed, offset + 2 + 2 * t, n) for t in range(n_mh)]).view(n_mh, n).cpu()
    return v0, z, u


@gpu
def test_native_draws_are_the_materialised_fields(cuda_device):
    dev, (n_mh, thin) = cuda_device, (7, 3)
    rejected = 0
    for kind, dim, n in [("double_well", 5, 37), ("harmonic", 100, 37), ("gmm", 32, 70), ("gaussian", 256, 9)]:
        spec, L, eps0 = energy_spec(kind, dim), 2, step_size(kind, dim)
        x0 = torch.randn(n, dim, generator=torch.Generator().manual_seed(5))
        seed, offset = 0x1234567887654321, 77
        v0, z, u = _fields(dev, seed, offset, n, dim, n_mh, TEMP)
        native = run_entry(dev, spec, x0, None, n_mh, thin, L, eps0, seed=seed, offset=offset)
        fed = run_entry(dev, spec, x0, v0, n_mh, thin, L, eps0, z=z, u=u)
        for key in ("x", "v", "traj", "accepted", "da", "eps_trace", "alpha_mean"):
            assert torch.equal(native[key], fed[key]), (kind, key)
            assert torch.isfinite(native[key].float()).all()
        rejected += int((~native["accepted"]).sum())
        # a sub-block of chains run alone (another grid, other lanes) reproduces its rows of the full launch
        lo, hi = n // 3, n // 3 + max(n // 2, 1)
        part = run_entry(dev, spec, x0[lo:hi], v0[lo:hi], n_mh, thin, L, eps0, z=z[:, lo:hi], u=u[:, lo:hi])
        for key in ("x", "v", "traj", "alpha_mean"):
            assert torch.equal(part[key], fed[key][lo:hi]), (kind, key)
        for key in ("accepted", "da", "eps_trace"):
            assert torch.equal(part[key], fed[key][:, lo:hi]), (kind, key)
    assert rejected > 0, "no proposal was rejected: the accept uniforms were not exercised"


# ---------------------------------------------------------------------------------
# 4. / 5. optional outputs, written rows and guards
# ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind,dim,n,n_mh,thin,L", [CASES["double_well"][1], CASES["harmonic"][6], CASES["gaussian"][2], CASES["rosenbrock"][2]])
def test_every_row_is_written_and_each_output_is_optional(cuda_device, kind, dim, n, n_mh, thin, L):
    c = case(kind, dim, n, n_mh, thin, L)
    got = _run_case(cuda_device, c)  # (run_entry checks the guard behind every output, and that every mask row is 0 / 1)
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
    # draw_v0: v is output only; init_da: da is output only -- every row written
    drawn = run_entry(cuda_device, c["spec"], c["x0"], None, n_mh, thin, L, c["eps0"], z=c["z"], u=c["u"], seed=3, offset=9)
    assert not bool((drawn["v"] == FILL).any()) and torch.isfinite(drawn["v"]).all() and not bool((drawn["da"] == FILL).any())


# ---------------------------------------------------------------------------------
# 6. wild coordinates
# ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind,dim,n,n_mh,thin,L", [CASES["double_well"][1], CASES["gaussian"][1]])
def test_wild_start_stays_in_its_chain(cuda_device, kind, dim, n, n_mh, thin, L):
    """A NaN coordinate in one chain and a 1e20 coordinate in another: every other chain's outputs, decisions and step sizes are
    bitwise the clean run's, and the wild chains' step sizes stay inside the bounds.  (The bounds hold up to the rounding of their
    logs to fp32, |log b| 2^-24 <= 4e-7 here, and of expf, 2 ulp: 1e-6 relative covers both.)"""
    c = case(kind, dim, n, n_mh, thin, L)
    bounds = (0.25 * c["eps0"], 4.0 * c["eps0"])
    x0 = c["x0"].clone()
    x0[3, 2] = float("nan")
    x0[7, 4] = 1e20
    got = run_entry(cuda_device, c["spec"], x0, c["v0"], n_mh, thin, L, c["eps0"], z=c["z"], u=c["u"], bounds=bounds)
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
    # alpha = NaN counted as 0: the NaN chain's iterate went down to the lower bound
    assert got["alpha_mean"][3] == 0 and math.isclose(got["eps_trace"][-1, 3].item(), bounds[0], rel_tol=1e-6)
    assert torch.isfinite(got["da"]).all()


# ---------------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------------
@gpu
def test_refusals_launch_nothing(cuda_device):
    """The refusals of test_adapt.py with real buffers: each raises its code and no buffer is touched."""
    from test_adapt import REFUSALS, _abi_call

    dev, (n, dim) = cuda_device, (4, 8)
    bufs = {name: torch.full((n, 260), FILL, device=dev) for name in ("x", "v", "da", "table", "trace", "alpha", "traj")}
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
# 8. through adapt_step_size
# ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("which", ["ghmc", "hmc"])
def test_adapt_step_size_is_one_launch(cuda_device, which):
    dev, (n, dim, k, L, eps0) = cuda_device, (300, 6, 40, 3, 0.02)
    spec = energy_spec("double_well", dim)
    if which == "ghmc":
        s, gamma, temp = ta.GeneralizedHMC(model_of(spec, dev), step_size=eps0, n_leapfrog_steps=L, friction=GAMMA, temperature=TEMP, device=dev), GAMMA, TEMP
    else:
        s, gamma, temp = ta.HamiltonianMonteCarlo(model_of(spec, dev), step_size=eps0, n_leapfrog_steps=L, device=dev), math.inf, 1.0
    x0 = torch.randn(n, dim, device=dev)
    keep = x0.clone()
    assert adapt.adapt_route(s, x0, gamma)[0] == "fused"
    g = torch.Generator(device=dev).manual_seed(5)
    before = dict(_lib.call_counts)
    r = s.adapt_step_size(x=x0, n_steps=k, generator=g, apply=False)
    torch.cuda.synchronize()
    new = {name: c - before.get(name, 0) for name, c in _lib.call_counts.items() if c != before.get(name, 0)}
    assert new == {ENTRY: 1}, new
    assert _rng._get_offset(g) == 4 * (2 * k + 1)
    assert torch.equal(x0, keep), "the caller's tensor was touched"
    assert s.get_scheduled_value("step_size") == eps0
    # the result is the entry's at the generator's coordinates
    want = run_entry(dev, spec, x0.cpu(), None, k, 1, L, eps0, gamma=gamma, temp=temp, seed=_rng.kernel_seed(5), offset=0)
    assert torch.equal(r.x.cpu(), want["x"]) and torch.equal(r.velocity.cpu(), want["v"]) and torch.equal(r.da.cpu(), want["da"])
    assert torch.equal(r.step_sizes.cpu(), want["da"][0]) and torch.equal(r.acceptance.cpu(), want["alpha_mean"])
    assert r.step_size.ndim == 0 and r.step_size.is_cuda and torch.allclose(r.step_size.cpu(), want["da"][0].log().median().exp(), rtol=1e-6)
    assert want["accepted"].any() and (~want["accepted"]).any() and float(r.step_size) > 2.0 * eps0
    # apply, with a passed velocity that stays untouched
    v0 = torch.randn(n, dim, device=dev)
    v_keep = v0.clone()
    r = s.adapt_step_size(x=x0, n_steps=k, velocity=v0, generator=g)
    assert torch.equal(v0, v_keep) and s.get_scheduled_value("step_size") == float(r.step_size)


@gpu
def test_other_configurations_take_the_eager_route_on_the_gpu(cuda_device):
    """A mass, a scheduler on the step size and a row wider than 256: the torch-op recurrence on the GPU, never the entry."""
    dev, (n, k, L) = cuda_device, (64, 8, 2)
    before = hip_calls(ENTRY)
    sched = lambda: ta.core.schedules.LinearScheduler(0.3, 0.1, 10)  # noqa: E731
    for cls in (ta.GeneralizedHMC, ta.HamiltonianMonteCarlo):
        for dim, kw in ((4, dict(step_size=0.1, mass=2.0)), (4, dict(step_size=sched())), (300, dict(step_size=0.1))):
            s = cls(ta.HarmonicModel(k=4.0, device=dev), n_leapfrog_steps=L, device=dev, **kw)
            x0 = 0.5 * torch.randn(n, dim, device=dev)
            assert adapt.adapt_route(s, x0, 1.0)[0] == "eager"
            r = s.adapt_step_size(x=x0, n_steps=k, generator=torch.Generator(device=dev).manual_seed(2))
            assert r.x.is_cuda and r.x.shape == (n, dim) and torch.isfinite(r.step_sizes).all() and float(r.step_size) > 0
    assert hip_calls(ENTRY) == before


# ---------------------------------------------------------------------------------
# 9. the law
# ---------------------------------------------------------------------------------
@gpu
def test_the_pooled_step_size_is_the_restatements(cuda_device):
    """energy_spec("harmonic", 4), a full refresh, L = 4, delta = 0.8, eps0 = 0.05, 4096 chains, 200 transitions: log step_size of
    the fused route (native draws) lies within 4.5 sqrt(se1^2 + se2^2) of the fp64 restatement's on torch draws,
    se = 1.2533 std(log eps-bar) / sqrt(n), each side's own."""
    dev, law = cuda_device, ac.LAW
    n, dim, k, L = law["n"], law["dim"], law["n_mh"], law["L"]
    spec = energy_spec(law["kind"], dim)
    g = torch.Generator().manual_seed(0)
    x0 = torch.randn(n, dim, generator=g)
    z, u = torch.randn(k, n, dim, generator=g), torch.rand(k, n, generator=g)
    ref = restate(to64(oracle_of(spec)), x0, torch.zeros(n, dim), z, u, law["eps0"], L, math.inf, 1.0, torch.float64, delta=law["delta"])
    s = ta.HamiltonianMonteCarlo(model_of(spec, dev), step_size=law["eps0"], n_leapfrog_steps=L, device=dev)
    before = hip_calls(ENTRY)
    r = s.adapt_step_size(x=x0.to(dev), n_steps=k, target_accept=law["delta"], generator=torch.Generator(device=dev).manual_seed(1))
    assert hip_calls(ENTRY) == before + 1
    got, se_got = ac.pooled_log(r.step_sizes.cpu())
    want, se_want = ac.pooled_log(ref["da"][0])
    bar = ac.LAW_SIGMAS * math.sqrt(se_got**2 + se_want**2)
    print(f"log step_size: fused {got:.5f} (se {se_got:.5f}), fp64 restatement {want:.5f} (se {se_want:.5f}), bar {bar:.5f}; "
          f"step sizes {math.exp(got):.4f} / {math.exp(want):.4f}; acceptance while adapting {r.acceptance.mean().item():.3f}")
    assert math.isclose(math.log(float(r.step_size)), got, abs_tol=1e-6)
    assert abs(got - want) < bar
    assert 0.7 < r.acceptance.mean().item() < 0.9
