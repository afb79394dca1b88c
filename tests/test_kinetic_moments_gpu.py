"""ebm_kinetic_moments_f32 on the GPU: the accumulators against the fp32 recurrences on the entry's own trajectories bit for bit,
the lean call, the final states against the plain chain entries (ebm_kinetic_chain_f32, ebm_ghmc_chain_f32) bit for bit and
against fp64 by the yardstick, the native draws against the materialised Philox fields, a sub-block of chains, what is written
and what is not, non-finite inputs, the accept counters, the refusals, and sample_moments of the two samplers on top of it."""

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib, _rng
from helpers import hip_calls, yardstick
from kinetic_cases import STEP, constants as baoab_constants
from kinetic_moments_cases import (CASES, ELEMENTWISE, GAMMA, GHMC_CASES, TEMP, baoab_case, energy_spec, ghmc_case, model_of, recip_table,
                                   v2_mean, welford)
from ghmc_cases import constants as ghmc_constants, step_size as ghmc_step

gpu = pytest.mark.gpu
ENTRY = "ebm_kinetic_moments_f32"
BAOAB, GHMC = 0, 1
FILL = 7.0
GUARD = 64  # elements behind every output that must keep FILL
# The BAOAB energy instantiation takes energy and gradient out of one evaluation (eval<true>); the plain entry evaluates the
# gradient alone (eval<false>).  For the mixture with up to 8 components these are two code paths of rows.h (eval_small against
# grad_only) that need not round alike: its final states are held by the yardstick, every other kind bit for bit.
ENERGY_PATH_DIFFERS = ("gmm",)


def _guarded(dev, shape, src=None, dtype=torch.float32, fill=FILL):
    """A tensor of `shape` in front of GUARD elements of FILL (in one allocation) -> (tensor, guard)."""
    numel = 1
    for s in shape:
        numel *= s
    buf = torch.full((numel + GUARD,), fill, device=dev, dtype=dtype)
    t = buf[:numel].view(shape)
    if src is not None:
        t.copy_(src)
    return t, buf[numel:]


def run_entry(dev, spec, sampler, x0, v0, k, burn_in, step, *, L=0, gamma=GAMMA, temp=TEMP, z=None, u=None, energy=True, v2=True,
              trajs=True, mask=True, counts=None, seed=0, offset=0):
    """One call of the entry -> dict of CPU tensors.  v0 None: draw_v0 = 1 and v starts from FILL.  Outputs start from FILL and
    sit in front of a guard: a slot the call did not write keeps it, and so must the guards."""
    n, dim = x0.shape
    h = (k - burn_in) // 2
    ghmc = sampler == GHMC
    model = model_of(spec, dev)
    g = {}
    x, g["x"] = _guarded(dev, (n, dim), x0)
    v, g["v"] = _guarded(dev, (n, dim), v0)
    mom, g["mom"] = _guarded(dev, (4, n, dim))
    e_mom, g["e_mom"] = _guarded(dev, (4, n)) if energy else (None, None)
    v2_mom, g["v2"] = _guarded(dev, (2, n, dim)) if (v2 and not ghmc) else (None, None)
    traj, g["traj"] = _guarded(dev, (n, 2 * h, dim)) if trajs else (None, None)
    e_traj, g["e_traj"] = _guarded(dev, (n, 2 * h)) if trajs else (None, None)
    v_traj, g["v_traj"] = _guarded(dev, (n, 2 * h, dim)) if (trajs and not ghmc) else (None, None)
    mk, g["mask"] = _guarded(dev, (k, n), dtype=torch.uint8) if (mask and ghmc) else (None, None)
    recip = recip_table(h).to(dev)
    z_d = None if z is None else z.to(dev).contiguous()
    u_d = None if u is None else u.to(dev).contiguous()
    before = hip_calls(ENTRY)
    _lib.call(ENTRY, model.fused_spec().to_c(), x.data_ptr(), v.data_ptr(), n, dim, sampler, k, burn_in, L, step, gamma, temp,
              int(v0 is None), recip.data_ptr(), mom.data_ptr(), _lib.ptr(e_mom), _lib.ptr(v2_mom), _lib.ptr(traj), _lib.ptr(e_traj),
              _lib.ptr(v_traj), _lib.ptr(mk), _lib.ptr(counts), _lib.ptr(z_d), _lib.ptr(u_d), seed, offset, _lib.stream_handle(dev))
    torch.cuda.synchronize()
    assert hip_calls(ENTRY) == before + 1
    for name, guard in g.items():
        assert guard is None or bool((guard == FILL).all()), f"the call wrote behind {name}"
    cpu = lambda t: None if t is None else t.cpu()  # noqa: E731
    out = {"x": cpu(x), "v": cpu(v), "mom": cpu(mom), "e_mom": cpu(e_mom), "v2": cpu(v2_mom), "traj": cpu(traj), "e_traj": cpu(e_traj),
           "v_traj": cpu(v_traj), "accepted": None, "h": h}
    if mk is not None:
        mk = mk.cpu()
        assert int(mk.max()) <= 1, "a row of the accept mask was not written"
        out["accepted"] = mk.bool()
    return out


def check_accumulators(got, energy=True):
    """mom, e_mom and v2_mom are the fp32 recurrences on the call's own trajectories, bit for bit; every slot was written."""
    h = got["h"]
    for key in ("x", "v", "mom", "traj") + (("e_mom", "e_traj") if energy else ()) + (("v2", "v_traj") if got["v2"] is not None else ()):
        assert not bool((got[key] == FILL).any()), f"a slot of {key} was not written"
    mean, m2 = welford(got["traj"], h)
    assert torch.equal(got["mom"][0], mean[0]) and torch.equal(got["mom"][2], mean[1])
    assert torch.equal(got["mom"][1], m2[0]) and torch.equal(got["mom"][3], m2[1])
    if energy:
        e_mean, e_m2 = welford(got["e_traj"], h)
        assert torch.equal(got["e_mom"][0], e_mean[0]) and torch.equal(got["e_mom"][2], e_mean[1])
        assert torch.equal(got["e_mom"][1], e_m2[0]) and torch.equal(got["e_mom"][3], e_m2[1])
    if got["v2"] is not None:
        assert torch.equal(got["v2"], v2_mean(got["v_traj"], h))
        assert torch.equal(got["v_traj"][:, -1], got["v"])
    assert torch.equal(got["traj"][:, -1], got["x"])


def same_outputs(a, b, keys=("x", "v", "mom", "e_mom", "v2")):
    for key in keys:
        assert (a[key] is None) == (b[key] is None), key
        assert a[key] is None or torch.equal(a[key], b[key]), key


def plain_baoab(dev, spec, x0, v0, k, step, z):
    n, dim = x0.shape
    x, v, z_d = x0.to(dev).clone(), v0.to(dev).clone(), z.to(dev).contiguous()
    _lib.call("ebm_kinetic_chain_f32", model_of(spec, dev).fused_spec().to_c(), x.data_ptr(), v.data_ptr(), n, dim, k, step, GAMMA, TEMP, 0,
              1, None, z_d.data_ptr(), 0, 0, _lib.stream_handle(dev))
    torch.cuda.synchronize()
    return x.cpu(), v.cpu()


def plain_ghmc(dev, spec, x0, v0, k, L, eps, z, u):
    n, dim = x0.shape
    x, v, z_d, u_d = x0.to(dev).clone(), v0.to(dev).clone(), z.to(dev).contiguous(), u.to(dev).contiguous()
    mask = torch.empty(k, n, dtype=torch.uint8, device=dev)
    _lib.call("ebm_ghmc_chain_f32", model_of(spec, dev).fused_spec().to_c(), x.data_ptr(), v.data_ptr(), n, dim, k, L, eps, GAMMA, TEMP, 0,
              1, None, mask.data_ptr(), z_d.data_ptr(), u_d.data_ptr(), 0, 0, _lib.stream_handle(dev))
    torch.cuda.synchronize()
    return x.cpu(), v.cpu(), mask.cpu().bool()


# ---------------------------------------------------------------------------------
# BAOAB, every kind
# ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind,dim,n,k,burn_in", CASES)
def test_baoab_cases_with_injected_draws(cuda_device, kind, dim, n, k, burn_in):
    dev, c = cuda_device, baoab_case(kind, dim, n, k, burn_in)
    run = lambda **kw: run_entry(dev, c["spec"], BAOAB, c["x0"], c["v0"], k, burn_in, c["h"], z=c["noise"], **kw)  # noqa: E731
    with_e, without_e = run(), run(energy=False)
    check_accumulators(with_e)
    check_accumulators(without_e, energy=False)
    assert bool((without_e["e_traj"] == FILL).all())  # no energy path: e_traj is not written
    # the call with no trajectory pointer returns the same states and moments
    same_outputs(run(trajs=False), with_e)
    same_outputs(run(trajs=False, energy=False), without_e)
    # the plain entry on the same draws: the same geometry, the same energy code, the same operations
    px, pv = plain_baoab(dev, c["spec"], c["x0"], c["v0"], k, c["h"], c["noise"])
    assert torch.equal(without_e["x"], px) and torch.equal(without_e["v"], pv)
    ref32, ref64 = c["ref32"], c["ref64"]
    if kind in ENERGY_PATH_DIFFERS:  # the factor test_kinetic_gpu.py gives the same recurrence
        print(yardstick(with_e["x"], ref32["x"], ref64["x"], k_med=1.5, what=f"kinetic moments (energy) x {kind} dim {dim}"))
        print(yardstick(with_e["v"], ref32["v"], ref64["v"], k_med=1.5, what=f"kinetic moments (energy) v {kind} dim {dim}"))
    else:
        assert torch.equal(with_e["x"], px) and torch.equal(with_e["v"], pv)
    if kind in ELEMENTWISE:  # ... and the restatement itself, positions and velocities of every counted step
        assert torch.equal(without_e["x"], ref32["x"]) and torch.equal(without_e["v"], ref32["v"])
        assert torch.equal(without_e["traj"], ref32["traj"][:, burn_in:])
    else:
        print(yardstick(without_e["x"], ref32["x"], ref64["x"], k_med=1.5, what=f"kinetic moments x {kind} dim {dim}"))
        print(yardstick(without_e["v"], ref32["v"], ref64["v"], k_med=1.5, what=f"kinetic moments v {kind} dim {dim}"))


# ---------------------------------------------------------------------------------
# generalized HMC, every kind
# ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind,dim,n,k,burn_in,L", GHMC_CASES)
def test_ghmc_cases_with_injected_draws(cuda_device, kind, dim, n, k, burn_in, L):
    dev, c = cuda_device, ghmc_case(kind, dim, n, k, burn_in, L)
    run = lambda **kw: run_entry(dev, c["spec"], GHMC, c["x0"], c["v0"], k, burn_in, c["eps"], L=L, z=c["z"], u=c["u"], **kw)  # noqa: E731
    got = run()
    check_accumulators(got)
    assert got["v2"] is None and got["v_traj"] is None
    same_outputs(run(trajs=False, mask=False), got)
    same_outputs(run(trajs=False, energy=False), got, keys=("x", "v", "mom"))
    ref32, ref64 = c["ref32"], c["ref64"]
    assert torch.equal(got["accepted"], ref32["accepted"])
    px, pv, pmask = plain_ghmc(dev, c["spec"], c["x0"], c["v0"], k, L, c["eps"], c["z"], c["u"])
    assert torch.equal(got["x"], px) and torch.equal(got["v"], pv) and torch.equal(got["accepted"], pmask)
    # a reject counts the held state again
    held = ~ref32["accepted"][burn_in + 1:].T  # [n, 2 h - 1]
    assert torch.equal((got["traj"][:, 1:] == got["traj"][:, :-1]).all(dim=2) | ~held, torch.ones_like(held))
    # the factor test_ghmc_gpu.py gives the same transition
    print(yardstick(got["x"], ref32["x"], ref64["x"], k_med=2.0, what=f"ghmc moments x {kind} dim {dim}"))
    print(yardstick(got["v"], ref32["v"], ref64["v"], k_med=2.0, what=f"ghmc moments v {kind} dim {dim}"))


@gpu
def test_accept_count_adds_to_what_it_held(cuda_device):
    dev = cuda_device
    kind, dim, n, k, burn_in, L = GHMC_CASES[1]
    c = ghmc_case(kind, dim, n, k, burn_in, L)
    counts, guard = _guarded(dev, (k,), dtype=torch.int32, fill=7)
    counts.fill_(100)
    got = run_entry(dev, c["spec"], GHMC, c["x0"], c["v0"], k, burn_in, c["eps"], L=L, z=c["z"], u=c["u"], counts=counts)
    assert bool((guard == 7).all())
    want = got["accepted"].sum(dim=1).to(torch.int32)
    assert torch.equal(counts.cpu(), 100 + want) and 0 < int(want.sum()) < k * n
    # several waves per transition (257 chains): one atomic per wave adds up
    kind, dim, n, k, burn_in, L = GHMC_CASES[0]
    c = ghmc_case(kind, dim, n, k, burn_in, L)
    counts = torch.zeros(k, dtype=torch.int32, device=dev)
    got = run_entry(dev, c["spec"], GHMC, c["x0"], c["v0"], k, burn_in, c["eps"], L=L, z=c["z"], u=c["u"], counts=counts, mask=True)
    assert torch.equal(counts.cpu(), got["accepted"].sum(dim=1).to(torch.int32))


# ---------------------------------------------------------------------------------
# native draws
# ---------------------------------------------------------------------------------
def _field(dev, kind, seed, step, n_elem):
    out = torch.empty((n_elem + 3) // 4 * 4, device=dev)
    _lib.call("ebm_noise_fill_f32", out.data_ptr(), n_elem, kind, seed, step, _lib.stream_handle(dev))
    return out[:n_elem].clone()


@gpu
def test_native_draws_are_the_materialised_fields(cuda_device):
    dev, (k, burn_in) = cuda_device, (11, 3)
    seed, offset = 0x1234567887654321, 77
    outputs = ("x", "v", "mom", "e_mom", "v2", "traj", "e_traj", "v_traj")
    rejected = 0
    for kind, dim, n in [("double_well", 5, 37), ("harmonic", 100, 37), ("gmm", 32, 70), ("gaussian", 256, 9)]:
        spec = energy_spec(kind, dim)
        x0 = torch.randn(n, dim, generator=torch.Generator().manual_seed(5))
        lo, hi = n // 3, n // 3 + max(n // 2, 1)
        # BAOAB: v0 at step offset, z at offset + 1 + s
        h = STEP[kind]
        v0 = (baoab_constants(h, GAMMA, TEMP)[3] * _field(dev, _lib.NOISE_NORMAL, seed, offset, n * dim)).view(n, dim).cpu()
        z = torch.stack([_field(dev, _lib.NOISE_NORMAL, seed, offset + 1 + s, n * dim) for s in range(k)]).view(k, n, dim).cpu()
        native = run_entry(dev, spec, BAOAB, x0, None, k, burn_in, h, seed=seed, offset=offset)
        fed = run_entry(dev, spec, BAOAB, x0, v0, k, burn_in, h, z=z)
        same_outputs(native, fed, outputs)
        assert all(torch.isfinite(native[key]).all() for key in outputs)
        mixed = run_entry(dev, spec, BAOAB, x0, None, k, burn_in, h, z=z, seed=seed, offset=offset)  # draw_v0 beside injected noise
        same_outputs(mixed, fed, outputs)
        # a sub-block of chains run alone (another grid, other lanes) reproduces its rows of the full launch
        part = run_entry(dev, spec, BAOAB, x0[lo:hi], v0[lo:hi], k, burn_in, h, z=z[:, lo:hi])
        for key in ("x", "v", "traj", "e_traj", "v_traj"):
            assert torch.equal(part[key], fed[key][lo:hi]), (kind, key)
        for key in ("mom", "e_mom", "v2"):
            assert torch.equal(part[key], fed[key][:, lo:hi]), (kind, key)
        # GHMC: v0 at step offset, z at offset + 1 + 2 t, u at offset + 2 + 2 t
        L, eps = 3, 2.0 * ghmc_step(kind, dim)
        v0 = (ghmc_constants(eps, L, GAMMA, TEMP)[2] * _field(dev, _lib.NOISE_NORMAL, seed, offset, n * dim)).view(n, dim).cpu()
        z = torch.stack([_field(dev, _lib.NOISE_NORMAL, seed, offset + 1 + 2 * t, n * dim) for t in range(k)]).view(k, n, dim).cpu()
        u = torch.stack([_field(dev, _lib.NOISE_UNIFORM, seed, offset + 2 + 2 * t, n) for t in range(k)]).view(k, n).cpu()
        native = run_entry(dev, spec, GHMC, x0, None, k, burn_in, eps, L=L, seed=seed, offset=offset)
        fed = run_entry(dev, spec, GHMC, x0, v0, k, burn_in, eps, L=L, z=z, u=u)
        same_outputs(native, fed, ("x", "v", "mom", "e_mom", "traj", "e_traj", "accepted"))
        rejected += int((~native["accepted"]).sum())
        for kw in (dict(z=z), dict(u=u)):  # either injected field alone: the rest still comes from the Philox fields
            mixed = run_entry(dev, spec, GHMC, x0, None, k, burn_in, eps, L=L, seed=seed, offset=offset, **kw)
            same_outputs(mixed, fed, ("x", "v", "mom", "e_mom", "accepted"))
        part = run_entry(dev, spec, GHMC, x0[lo:hi], v0[lo:hi], k, burn_in, eps, L=L, z=z[:, lo:hi], u=u[:, lo:hi])
        for key in ("x", "v", "traj", "e_traj"):
            assert torch.equal(part[key], fed[key][lo:hi]), (kind, key)
        for key in ("mom", "e_mom", "accepted"):
            assert torch.equal(part[key], fed[key][:, lo:hi]), (kind, key)
    assert rejected > 0, "no proposal was rejected: the accept uniforms were not exercised"


# ---------------------------------------------------------------------------------
# non-finite inputs
# ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("sampler", [BAOAB, GHMC])
@pytest.mark.parametrize("which", [1, 7])  # double well dim 5, gaussian dim 5: 37 chains, (11, 3)
def test_wild_start_stays_in_its_chain(cuda_device, sampler, which):
    """A NaN coordinate in one chain and a 1e20 coordinate in another: every other chain's outputs are bitwise the clean run's."""
    dev = cuda_device
    if sampler == BAOAB:
        kind, dim, n, k, burn_in = CASES[which]
        c = baoab_case(kind, dim, n, k, burn_in)
        run = lambda x0: run_entry(dev, c["spec"], BAOAB, x0, c["v0"], k, burn_in, c["h"], z=c["noise"])  # noqa: E731
    else:
        kind, dim, n, k, burn_in, L = GHMC_CASES[which]
        c = ghmc_case(kind, dim, n, k, burn_in, L)
        run = lambda x0: run_entry(dev, c["spec"], GHMC, x0, c["v0"], k, burn_in, c["eps"], L=L, z=c["z"], u=c["u"])  # noqa: E731
    assert (dim, n) == (5, 37)
    x0 = c["x0"].clone()
    x0[3, 2] = float("nan")
    x0[7, 4] = 1e20
    got, clean = run(x0), run(c["x0"])
    others = [i for i in range(n) if i not in (3, 7)]
    for key in ("x", "v", "traj", "e_traj") + (("v_traj",) if sampler == BAOAB else ()):
        assert torch.isfinite(clean[key]).all()
        assert torch.equal(got[key][others], clean[key][others]), key
    for key in ("mom", "e_mom") + (("v2",) if sampler == BAOAB else ("accepted",)):
        assert torch.equal(got[key][:, others], clean[key][:, others]), key
    assert torch.isnan(got["mom"][:, 3]).any()


# ---------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------
@gpu
def test_refusals_launch_nothing(cuda_device):
    """The refusals of test_kinetic_moments.py with real buffers: each raises its code and no buffer is touched."""
    from test_kinetic_moments import REFUSALS, _abi_call

    dev, (n, dim) = cuda_device, (4, 8)
    bufs = {name: torch.full((4 * n, 260), FILL, device=dev) for name in ("x", "v", "mom", "recip", "v2_mom", "v_traj")}
    real = {name: bufs[name].data_ptr() for name in ("x", "v", "mom", "recip")}
    desc = model_of(energy_spec("double_well", dim), dev).fused_spec().to_c()
    for kw, exc, match in REFUSALS:
        kw = {key: (bufs[key].data_ptr() if key in ("v2_mom", "v_traj") and val is not None else val) for key, val in kw.items()}
        with pytest.raises(exc, match=match):
            _abi_call(desc, **{**real, **kw})
    mlp = ta.MLPEnergy(dim, 64, device=dev)
    with pytest.raises(RuntimeError, match=r"code -2"):
        _abi_call(mlp.fused_spec().to_c(), **real)
    torch.cuda.synchronize()
    for t in bufs.values():
        assert bool((t == FILL).all())


# ---------------------------------------------------------------------------------
# through the samplers
# ---------------------------------------------------------------------------------
def _sampler(which, dev, model, step, L=3, gamma=GAMMA, temp=TEMP):
    if which == "baoab":
        return ta.UnderdampedLangevin(model, step_size=step, friction=gamma, temperature=temp, device=dev)
    return ta.GeneralizedHMC(model, step_size=step, n_leapfrog_steps=L, friction=gamma, temperature=temp, device=dev)


@gpu
@pytest.mark.parametrize("which", ["baoab", "ghmc"])
def test_sample_moments_is_one_launch(cuda_device, which, monkeypatch):
    dev, (n, dim, k, burn_in, step) = cuda_device, (300, 6, 40, 5, 0.05)  # (an odd count: one more step is burnt)
    spec = energy_spec("double_well", dim)
    s = _sampler(which, dev, model_of(spec, dev), step)
    g0 = torch.Generator().manual_seed(9)
    x0 = torch.randn(n, dim, generator=g0).to(dev)
    v0 = torch.randn(n, dim, generator=g0).to(dev)
    keep_x, keep_v = x0.clone(), v0.clone()
    assert s._route(x0)[0] == "fused"
    g = torch.Generator(device=dev).manual_seed(5)
    before = dict(_lib.call_counts)
    x, mom, v = s.sample_moments(x=x0, n_steps=k, burn_in=burn_in, energy=True, return_velocity=True, generator=g)
    torch.cuda.synchronize()
    new = {name: c - before.get(name, 0) for name, c in _lib.call_counts.items() if c != before.get(name, 0)}
    assert new == {ENTRY: 1}, new
    # the generator advanced as sample() advances it, and the states are sample()'s for the same seed
    steps = (2 * k if which == "ghmc" else k) + 1
    assert _rng._get_offset(g) == 4 * steps
    g2 = torch.Generator(device=dev).manual_seed(5)
    xs, vs = s.sample(x=x0, n_steps=k, return_velocity=True, generator=g2)
    assert _rng._get_offset(g2) == _rng._get_offset(g)
    assert torch.equal(x, xs) and torch.equal(v, vs)
    assert torch.equal(x0, keep_x), "the caller's tensor was touched"
    # ... and the entry's at the generator's coordinates
    sampler_id = GHMC if which == "ghmc" else BAOAB
    want = run_entry(dev, spec, sampler_id, x0.cpu(), None, k, 6, step, L=3, seed=_rng.kernel_seed(5), offset=0)
    assert torch.equal(x.cpu(), want["x"]) and torch.equal(v.cpu(), want["v"])
    assert mom.half_len == 17 and mom.n_nonfinite == 0
    assert torch.equal(mom.chain_mean.cpu(), want["mom"][[0, 2]]) and torch.equal(mom.chain_m2.cpu(), want["mom"][[1, 3]])
    assert torch.equal(mom.energy_mean.cpu(), want["e_mom"][[0, 2]]) and torch.equal(mom.energy_m2.cpu(), want["e_mom"][[1, 3]])
    if which == "baoab":
        assert torch.equal(mom.velocity_sq_mean.cpu(), want["v2"]) and mom.acceptance_rate is None
        assert mom.kinetic_temperature.shape == (dim,)
    else:
        assert mom.velocity_sq_mean is None and mom.kinetic_temperature is None
        assert torch.allclose(mom.acceptance_rate.cpu(), want["accepted"].float().mean(dim=1), rtol=0, atol=1e-6)
        # the entry's counters, which the sampler falls to when the mask would be too large, give the same rates
        from torchebm_amd.samplers import kinetic_moments

        monkeypatch.setattr(kinetic_moments, "MASK_MAX_BYTES", 0)
        _, counted = s.sample_moments(x=x0, n_steps=k, burn_in=burn_in, generator=torch.Generator(device=dev).manual_seed(5))
        assert torch.equal(counted.acceptance_rate, mom.acceptance_rate) and torch.equal(counted.chain_mean, mom.chain_mean)
    assert torch.isfinite(mom.rhat).all() and torch.isfinite(mom.ess).all() and torch.isfinite(mom.energy_rhat)
    # a passed velocity is continued and never written
    x, mom, v = s.sample_moments(x=x0, n_steps=8, velocity=v0, return_velocity=True, generator=torch.Generator(device=dev).manual_seed(6))
    xs, vs = s.sample(x=x0, n_steps=8, velocity=v0, return_velocity=True, generator=torch.Generator(device=dev).manual_seed(6))
    assert torch.equal(v0, keep_v) and torch.equal(x0, keep_x) and torch.equal(x, xs) and torch.equal(v, vs)
    assert mom.energy_mean is None


@gpu
@pytest.mark.parametrize("which", ["baoab", "ghmc"])
def test_the_harmonic_laws_hold_on_the_fused_route(cuda_device, which):
    from test_kinetic_moments import LAW, LAW_GHMC_L, check_baoab_law, check_ghmc_law, law_start

    dev = cuda_device
    s = _sampler(which, dev, ta.HarmonicModel(k=LAW["k"], device=dev), LAW["step"], L=LAW_GHMC_L, gamma=LAW["gamma"], temp=LAW["temp"])
    before = hip_calls(ENTRY)
    _, mom = s.sample_moments(x=law_start(dev), n_steps=LAW["n_steps"], burn_in=LAW["burn_in"],
                              generator=torch.Generator(device=dev).manual_seed(LAW["seed"]))
    assert hip_calls(ENTRY) == before + 1
    (check_baoab_law if which == "baoab" else check_ghmc_law)(mom)


@gpu
@pytest.mark.parametrize("which", ["baoab", "ghmc"])
def test_a_module_energy_takes_the_eager_route_on_the_gpu(cuda_device, which):
    """An nn.Module energy: the torch-op route on the GPU with its own draws; the pooled variance agrees with the CPU eager
    route's within the 3 % docs/design/moments.md reports for its cross-device check."""

    class Quadratic(ta.BaseModel):
        def forward(self, x):
            return 2.0 * (x**2).sum(dim=-1)

    dev, (n, dim, k, burn_in) = cuda_device, (4096, 2, 120, 20)
    x0 = 0.5 * torch.randn(n, dim, generator=torch.Generator().manual_seed(1))
    before = hip_calls(ENTRY)
    s = _sampler(which, dev, Quadratic().to(dev), 0.3, gamma=1.0, temp=1.0)
    x, mom = s.sample_moments(x=x0.to(dev), n_steps=k, burn_in=burn_in, generator=torch.Generator(device=dev).manual_seed(2))
    assert hip_calls(ENTRY) == before and x.is_cuda and mom.chain_mean.is_cuda
    cpu = _sampler(which, "cpu", Quadratic(), 0.3, gamma=1.0, temp=1.0)
    _, want = cpu.sample_moments(x=x0, n_steps=k, burn_in=burn_in, generator=torch.Generator().manual_seed(2))
    rel = (mom.var.cpu() / want.var - 1.0).abs()
    print("eager on the GPU against eager on the CPU, pooled variance:", mom.var.tolist(), want.var.tolist())
    assert (rel < 0.03).all(), rel
