"""ebm_ghmc_chain_f32 on the GPU: the transition against the restatement of ghmc_cases.py (decisions exactly, states by the fp64
yardstick), the flip bit for bit, the transition against ebm_hmc_chain_f32, the native draws against the materialised Philox
fields, a run cut in two, what is written and what is not, non-finite inputs, the refusals, and GeneralizedHMC on top of it."""

import math

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib, _rng
from helpers import hip_calls, yardstick
from ghmc_cases import (ALL_CASES, CASES, GAMMA, LAW_SEED, LAW_SHAPE, LAW_STEPS, LAWS, TEMP, case, constants, energy_spec, leapfrog_steps,
                        model_of, step_size)

gpu = pytest.mark.gpu
ENTRY = "ebm_ghmc_chain_f32"
FILL = 7.0
GUARD = 64  # elements behind every output that must keep FILL


def _guarded(dev, shape, src=None, dtype=torch.float32):
    """A tensor of `shape` in front of GUARD elements of FILL (in one allocation) -> (tensor, guard)."""
    numel = 1
    for s in shape:
        numel *= s
    buf = torch.full((numel + GUARD,), FILL, device=dev, dtype=dtype)
    t = buf[:numel].view(shape)
    if src is not None:
        t.copy_(src)
    return t, buf[numel:]


def run_entry(dev, spec, x0, v0, n_mh, thin, L, eps, *, gamma=GAMMA, temp=TEMP, z=None, u=None, traj=True, mask=True, seed=0, offset=0):
    """One call of the entry -> dict of CPU tensors x, v [n, dim], traj [n, n_mh // thin, dim], accepted [n_mh, n].  v0 None:
    draw_v0 = 1 and v starts from FILL.  Outputs start from FILL and sit in front of a guard: a slot the call did not write keeps
    it, and so must the guards."""
    n, dim = x0.shape
    model = model_of(spec, dev)
    x, gx = _guarded(dev, (n, dim), x0)
    v, gv = _guarded(dev, (n, dim), v0)
    tr, gt = _guarded(dev, (n, n_mh // thin, dim)) if traj else (None, None)
    mk, gm = _guarded(dev, (n_mh, n), dtype=torch.uint8) if mask else (None, None)
    z_d = None if z is None else z.to(dev).contiguous()
    u_d = None if u is None else u.to(dev).contiguous()
    before = hip_calls(ENTRY)
    _lib.call(ENTRY, model.fused_spec().to_c(), x.data_ptr(), v.data_ptr(), n, dim, n_mh, L, eps, gamma, temp, int(v0 is None), thin,
              _lib.ptr(tr), _lib.ptr(mk), _lib.ptr(z_d), _lib.ptr(u_d), seed, offset, _lib.stream_handle(dev))
    torch.cuda.synchronize()
    assert hip_calls(ENTRY) == before + 1
    for guard in (gx, gv, gt, gm):
        assert guard is None or bool((guard == FILL).all()), "the call wrote behind an output"
    out = {"x": x.cpu(), "v": v.cpu(), "traj": None if tr is None else tr.cpu(), "accepted": None}
    if mask:
        mk = mk.cpu()
        assert int(mk.max()) <= 1, "a row of the accept mask was not written"
        out["accepted"] = mk.bool()
    return out


def _run_case(dev, c, **kw):
    return run_entry(dev, c["spec"], c["x0"], c["v0"], c["n_mh"], c["thin"], c["L"], c["eps"], gamma=c["gamma"], temp=c["temp"], z=c["z"],
                     u=c["u"], **kw)


# ---------------------------------------------------------------------------------
# the transition, every kind
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
    # the factor test_tempering_hmc_gpu.py gives the same trajectory code
    print(yardstick(got["x"], ref32["x"], ref64["x"], k_med=2.0, what=f"ghmc x {kind} dim {dim}"))
    print(yardstick(got["v"], ref32["v"], ref64["v"], k_med=2.0, what=f"ghmc v {kind} dim {dim}"))
    print(yardstick(rows(got["traj"]), rows(ref32["traj"]), rows(ref64["traj"]), k_med=2.0, what=f"ghmc traj {kind} dim {dim}"))
    if n_mh % thin == 0:
        assert torch.equal(got["traj"][:, -1], got["x"])


@gpu
@pytest.mark.parametrize("kind", list(CASES))
def test_every_group_accepts_and_rejects(kind):
    acc = torch.cat([case(*c)["ref32"]["accepted"].flatten() for c in CASES[kind]])
    assert acc.any() and (~acc).any()


@gpu
@pytest.mark.parametrize("kind", ["double_well", "gmm"])
@pytest.mark.parametrize("dim", [5, 100])
def test_the_flip_bit_for_bit(cuda_device, kind, dim):
    """u = 1 is never below a <= 1: every proposal is rejected, x stays and v = -(c1 v0 + c2 z), each operation rounded on its own."""
    n, L, eps = 37, leapfrog_steps(dim), step_size(kind, dim)
    g = torch.Generator().manual_seed(31)
    x0, v0, z = torch.randn(n, dim, generator=g), torch.randn(n, dim, generator=g), torch.randn(1, n, dim, generator=g)
    got = run_entry(cuda_device, energy_spec(kind, dim), x0, v0, 1, 1, L, eps, z=z, u=torch.ones(1, n))
    c1, c2, _, _ = constants(eps, L, GAMMA, TEMP)
    assert not got["accepted"].any()
    assert torch.equal(got["x"], x0) and torch.equal(got["traj"][:, 0], x0)
    assert torch.equal(got["v"], -(c1 * v0 + c2 * z[0]))


@gpu
@pytest.mark.parametrize("dim", [5, 100])
def test_the_transition_is_the_hmc_kernels(cuda_device, dim):
    """gamma = inf, T = 1: c1 = 0, c2 = beta = 1 -- the chains are ebm_hmc_chain_f32 chains, bit for bit (double well at dims
    where that entry runs the lane-group kernel of the same geometry; the call test_tempering_hmc_gpu.py makes)."""
    dev, (n, n_mh, L, eps) = cuda_device, (111, 5, 4, 0.15)
    spec = energy_spec("double_well", dim)
    g = torch.Generator().manual_seed(21)
    x0, v0 = torch.randn(n, dim, generator=g), torch.randn(n, dim, generator=g)
    z, u = torch.randn(n_mh, n, dim, generator=g), torch.rand(n_mh, n, generator=g)
    got = run_entry(dev, spec, x0, v0, n_mh, 1, L, eps, gamma=math.inf, temp=1.0, z=z, u=u)
    rows, p_d, u_d = x0.to(dev).clone(), z.to(dev), u.to(dev)
    mask = torch.empty(n_mh, n, dtype=torch.uint8, device=dev)
    _lib.call("ebm_hmc_chain_f32", model_of(spec, dev).fused_spec().to_c(), rows.data_ptr(), n, dim, n_mh, L, eps, None, 0, 0.0,
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


def _fields(dev, seed, offset, n, dim, n_mh, eps, L):
    """v0, z, u of a call at (seed, offset): step `offset` scaled by sqrt_temp, normals at offset + 1 + 2 t, uniforms at
    offset + 2 + 2 t."""
    sqrt_temp = constants(eps, L, GAMMA, TEMP)[2]
    v0 = (sqrt_temp * _field(dev, _lib.NOISE_NORMAL, seed, offset, n * dim)).view(n, dim).cpu()
    z = torch.stack([_field(dev, _lib.NOISE_NORMAL, seed, offset + 1 + 2 * t, n * dim) for t in range(n_mh)]).view(n_mh, n, dim).cpu()
    u = torch.stack([_field(dev, _lib.NOISE_UNIFORM, seed, offset + 2 + 2 * t, n) for t in range(n_mh)]).view(n_mh, n).cpu()
    return v0, z, u


@gpu
def test_native_draws_are_the_materialised_fields(cuda_device):
    dev, (n_mh, thin) = cuda_device, (7, 3)
    rejected = 0
    for kind, dim, n in [("double_well", 5, 37), ("harmonic", 100, 37), ("gmm", 32, 70), ("gaussian", 256, 9)]:
        spec, L, eps = energy_spec(kind, dim), leapfrog_steps(dim), 2.0 * step_size(kind, dim)
        x0 = torch.randn(n, dim, generator=torch.Generator().manual_seed(5))
        seed, offset = 0x1234567887654321, 77
        v0, z, u = _fields(dev, seed, offset, n, dim, n_mh, eps, L)
        native = run_entry(dev, spec, x0, None, n_mh, thin, L, eps, seed=seed, offset=offset)
        fed = run_entry(dev, spec, x0, v0, n_mh, thin, L, eps, z=z, u=u)
        for key in ("x", "v", "traj", "accepted"):
            assert torch.equal(native[key], fed[key]), (kind, key)
            assert torch.isfinite(native[key].float()).all()
        rejected += int((~native["accepted"]).sum())
        # either injected field alone, and draw_v0 beside injected draws: the rest still comes from the Philox fields
        for kw in (dict(z=z), dict(u=u), dict(z=z, u=u)):
            mixed = run_entry(dev, spec, x0, None, n_mh, thin, L, eps, seed=seed, offset=offset, **kw)
            assert torch.equal(mixed["x"], fed["x"]) and torch.equal(mixed["v"], fed["v"]), (kind, sorted(kw))
        # a sub-block of chains run alone (another grid, other lanes) reproduces its rows of the full launch
        lo, hi = n // 3, n // 3 + max(n // 2, 1)
        part = run_entry(dev, spec, x0[lo:hi], v0[lo:hi], n_mh, thin, L, eps, z=z[:, lo:hi], u=u[:, lo:hi])
        for key in ("x", "v", "traj"):
            assert torch.equal(part[key], fed[key][lo:hi]), (kind, key)
        assert torch.equal(part["accepted"], fed["accepted"][:, lo:hi])
    assert rejected > 0, "no proposal was rejected: the accept uniforms were not exercised"


@gpu
@pytest.mark.parametrize("kind", ["double_well", "gmm"])
@pytest.mark.parametrize("dim", [5, 100])
def test_two_calls_are_one(cuda_device, kind, dim):
    """(n1, offset) then (n2, offset + 2 n1) with draw_v0 = 0 is one call of n1 + n2: the carried energy and force are
    re-evaluated by the evaluation the last leapfrog step ended on."""
    dev, (n, n1, n2) = cuda_device, (37, 4, 7)
    spec, L, eps = energy_spec(kind, dim), leapfrog_steps(dim), 2.0 * step_size(kind, dim)
    x0 = torch.randn(n, dim, generator=torch.Generator().manual_seed(6))
    seed, offset = 0x0123456789ABCDEF, 41
    whole = run_entry(dev, spec, x0, None, n1 + n2, 1, L, eps, seed=seed, offset=offset)
    first = run_entry(dev, spec, x0, None, n1, 1, L, eps, seed=seed, offset=offset)
    second = run_entry(dev, spec, first["x"], first["v"], n2, 1, L, eps, seed=seed, offset=offset + 2 * n1)
    assert torch.equal(second["x"], whole["x"]) and torch.equal(second["v"], whole["v"])
    assert torch.equal(torch.cat((first["traj"], second["traj"]), dim=1), whole["traj"])
    assert torch.equal(torch.cat((first["accepted"], second["accepted"])), whole["accepted"])


# ---------------------------------------------------------------------------------
# what is written
# ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind,dim,n,n_mh,thin,L", [CASES["double_well"][1], CASES["harmonic"][6], CASES["gaussian"][2], CASES["rosenbrock"][2]])
def test_every_row_is_written_and_nothing_else(cuda_device, kind, dim, n, n_mh, thin, L):
    c = case(kind, dim, n, n_mh, thin, L)
    got = _run_case(cuda_device, c)  # (run_entry checks the guards behind x, v, traj and the mask, and that every mask row is 0 / 1)
    lean = _run_case(cuda_device, c, traj=False, mask=False)
    assert lean["traj"] is None and lean["accepted"] is None and torch.equal(lean["x"], got["x"]) and torch.equal(lean["v"], got["v"])
    for key in ("x", "v", "traj"):
        assert not bool((got[key] == FILL).any()), f"a slot of {key} was not written"
    # draw_v0: v is output only, every row written
    drawn = run_entry(cuda_device, c["spec"], c["x0"], None, n_mh, thin, L, c["eps"], z=c["z"], u=c["u"], seed=3, offset=9)
    assert not bool((drawn["v"] == FILL).any()) and torch.isfinite(drawn["v"]).all()


# ---------------------------------------------------------------------------------
# non-finite inputs
# ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind,dim,n,n_mh,thin,L", [CASES["double_well"][1], CASES["gaussian"][1]])
def test_wild_start_stays_in_its_chain(cuda_device, kind, dim, n, n_mh, thin, L):
    """A NaN coordinate in one chain and a 1e20 coordinate in another (ordinary non-finite arithmetic: NaN energies reject): every
    other chain's outputs and decisions are bitwise the clean run's."""
    c = case(kind, dim, n, n_mh, thin, L)
    x0 = c["x0"].clone()
    x0[3, 2] = float("nan")
    x0[7, 4] = 1e20
    got = run_entry(cuda_device, c["spec"], x0, c["v0"], n_mh, thin, L, c["eps"], z=c["z"], u=c["u"])
    clean = _run_case(cuda_device, c)
    others = [i for i in range(n) if i not in (3, 7)]
    for key in ("x", "v", "traj"):
        assert torch.isfinite(clean[key]).all()
        assert torch.equal(got[key][others], clean[key][others]), key
    assert torch.equal(got["accepted"][:, others], clean["accepted"][:, others])
    assert torch.isnan(got["x"][3]).any() and not got["accepted"][:, 3].any()  # the NaN chain held its state and only flipped


# ---------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------
@gpu
def test_refusals_launch_nothing(cuda_device):
    """The refusals of test_ghmc.py with real buffers: each raises its code and no buffer is touched."""
    from test_ghmc import REFUSALS, _abi_call

    dev, (n, dim) = cuda_device, (4, 8)
    x = torch.full((n, 260), FILL, device=dev)
    v = torch.full((n, 260), FILL, device=dev)
    real = dict(x=x.data_ptr(), v=v.data_ptr())
    desc = model_of(energy_spec("double_well", dim), dev).fused_spec().to_c()
    for kw, exc, match in REFUSALS:
        with pytest.raises(exc, match=match):
            _abi_call(desc, **{**real, **kw})
    mlp = ta.MLPEnergy(dim, 64, device=dev)
    with pytest.raises(RuntimeError, match=r"code -2"):
        _abi_call(mlp.fused_spec().to_c(), **real)
    torch.cuda.synchronize()
    for t in (x, v):
        assert bool((t == FILL).all())


# ---------------------------------------------------------------------------------
# through GeneralizedHMC.sample()
# ---------------------------------------------------------------------------------
@gpu
def test_sample_is_one_launch(cuda_device):
    dev, (n, dim, k1, k2, L, eps) = cuda_device, (300, 6, 17, 23, 3, 0.2)
    k = k1 + k2
    x0 = torch.randn(n, dim, device=dev)
    keep = x0.clone()
    spec = energy_spec("double_well", dim)
    s = ta.GeneralizedHMC(model_of(spec, dev), step_size=eps, n_leapfrog_steps=L, friction=GAMMA, temperature=TEMP, device=dev)
    assert s._route(x0)[0] == "fused"
    g = torch.Generator(device=dev).manual_seed(5)
    before = dict(_lib.call_counts)
    x, v = s.sample(x=x0, n_steps=k, return_velocity=True, generator=g)
    torch.cuda.synchronize()
    new = {name: c - before.get(name, 0) for name, c in _lib.call_counts.items() if c != before.get(name, 0)}
    assert new == {ENTRY: 1}, new
    assert _rng._get_offset(g) == 4 * (2 * k + 1)
    assert torch.equal(x0, keep), "the caller's tensor was touched"
    assert x.is_cuda and v.is_cuda and x.shape == v.shape == (n, dim) and torch.isfinite(x).all() and torch.isfinite(v).all()
    # the states are the entry's at the generator's coordinates
    want = run_entry(dev, spec, x0.cpu(), None, k, 1, L, eps, seed=_rng.kernel_seed(5), offset=0)
    assert torch.equal(x.cpu(), want["x"]) and torch.equal(v.cpu(), want["v"])
    assert want["accepted"].any() and (~want["accepted"]).any()
    # cut in two: the second call continues from the returned velocity at the Philox step the first one stopped at
    g = torch.Generator(device=dev).manual_seed(5)
    xa, va = s.sample(x=x0, n_steps=k1, return_velocity=True, generator=g)
    assert _rng._get_offset(g) == 4 * (2 * k1 + 1)
    _rng._set_offset(g, 4 * 2 * k1)  # (a call owns 2 k + 1 steps; the uncut run drew step 2 k1 + 1 + 2 t where this one draws its step 1 + 2 t)
    va_keep = va.clone()
    xb, vb = s.sample(x=xa, n_steps=k2, velocity=va, return_velocity=True, reset_schedulers=False, generator=g)
    assert torch.equal(va, va_keep), "the caller's velocity was touched"
    assert torch.equal(xb, x) and torch.equal(vb, v)
    # trajectory and diagnostics: the kept positions, their statistics and the acceptance of the kept transitions
    traj, diag = s.sample(x=x0, n_steps=k, thin=4, return_trajectory=True, return_diagnostics=True,
                          generator=torch.Generator(device=dev).manual_seed(5))
    assert traj.shape == (n, k // 4, dim) and torch.equal(traj[:, -1], x)
    assert diag["mean"].shape == diag["var"].shape == (k // 4, dim) and diag["energy"].shape == diag["acceptance_rate"].shape == (k // 4,)
    assert torch.allclose(diag["mean"], traj.mean(dim=0), atol=1e-5)
    assert torch.allclose(diag["var"], traj.var(dim=0, unbiased=False), rtol=1e-4, atol=1e-6)
    assert torch.allclose(diag["energy"], torch.stack([s.model(traj[:, j].contiguous()).mean() for j in range(k // 4)]), rtol=1e-4)
    # (accepted / 300 formed on two devices: a count apart is 3e-3)
    assert torch.allclose(diag["acceptance_rate"].cpu(), want["accepted"][3::4][: k // 4].float().mean(dim=1), rtol=0, atol=1e-6)
    assert torch.allclose(diag["kinetic_temperature"], v.square().mean())


@gpu
def test_other_configurations_take_the_eager_route_on_the_gpu(cuda_device):
    """A scheduler on the step size and a row wider than 256: the torch-op recurrence on the GPU, fed the CPU run's draws, lands
    where the CPU run does within the bars the HMC fixtures use (5e-4 for 99 % of the chains, 5e-3 for every one)."""
    dev, (n, n_mh, L) = cuda_device, (64, 6, 2)
    before = hip_calls(ENTRY)
    for dim, step in ((4, lambda: ta.core.schedules.LinearScheduler(0.3, 0.1, 10)), (300, lambda: 0.1)):
        g = torch.Generator().manual_seed(2)
        x0 = 0.5 * torch.randn(n, dim, generator=g)
        cpu = ta.GeneralizedHMC(ta.HarmonicModel(k=4.0), step_size=step(), n_leapfrog_steps=L)
        draws = []
        cpu._draw_normal = lambda shape, like, gen: draws.append(torch.randn(shape, generator=gen)) or draws[-1]
        cpu._draw_uniform = lambda m, like, gen: draws.append(torch.rand(m, generator=gen)) or draws[-1]
        want_x, want_v = cpu.sample(x=x0, n_steps=n_mh, return_velocity=True, generator=g)
        assert len(draws) == 1 + 2 * n_mh
        s = ta.GeneralizedHMC(ta.HarmonicModel(k=4.0, device=dev), step_size=step(), n_leapfrog_steps=L, device=dev)
        assert s._route(x0.to(dev))[0] == "eager"
        replay = iter(draws)
        s._draw_normal = lambda shape, like, gen: next(replay).to(dev)
        s._draw_uniform = lambda m, like, gen: next(replay).to(dev)
        x, v = s.sample(x=x0.to(dev), n_steps=n_mh, return_velocity=True)
        assert x.is_cuda and v.is_cuda and x.shape == (n, dim)
        for got, want in ((x, want_x), (v, want_v)):
            err = ((got.cpu() - want).abs() / want.abs().clamp(min=1.0)).amax(dim=1)
            assert (err <= 5e-4).float().mean().item() >= 0.99 and err.max().item() <= 5e-3, (dim, err.max().item())
    assert hip_calls(ENTRY) == before


@gpu
def test_the_harmonic_law_holds_on_the_fused_route(cuda_device):
    from test_ghmc import check_harmonic_law, law_start

    dev, (n, dim) = cuda_device, LAW_SHAPE
    k_spring, eps, gamma, temp, L = LAWS[0]
    s = ta.GeneralizedHMC(ta.HarmonicModel(k=k_spring, device=dev), step_size=eps, n_leapfrog_steps=L, friction=gamma, temperature=temp,
                          device=dev)
    before = hip_calls(ENTRY)
    x, diag, v = s.sample(x=law_start(n, dim, k_spring, temp, LAW_SEED, dev), n_steps=LAW_STEPS, thin=LAW_STEPS // 4,
                          return_diagnostics=True, return_velocity=True, generator=torch.Generator(device=dev).manual_seed(LAW_SEED))
    assert hip_calls(ENTRY) == before + 1
    check_harmonic_law(x.cpu(), v.cpu(), {key: val.cpu() for key, val in diag.items()}, k_spring, temp)
