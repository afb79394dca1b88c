"""ebm_kinetic_chain_f32 on the GPU: the BAOAB recurrence against the restatement of kinetic_cases.py (bit for bit for the
element-wise energies, within the reference's own fp32 error for the coupled ones), the native draws against the materialised
Philox fields, a run cut in two, what is written and what is not, non-finite inputs, the refusals, and UnderdampedLangevin on
top of it."""

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib, _rng
from helpers import hip_calls, yardstick
from kinetic_cases import COUPLED_CASES, EXACT_CASES, GAMMA, STEP, TEMP, case, constants, energy_spec, model_of

gpu = pytest.mark.gpu
ENTRY = "ebm_kinetic_chain_f32"
FILL = 7.0
GUARD = 64  # floats behind every output that must keep FILL


def _guarded(dev, shape, src=None):
    """A tensor of `shape` in front of GUARD floats of FILL (in one allocation) -> (tensor, guard)."""
    numel = 1
    for s in shape:
        numel *= s
    buf = torch.full((numel + GUARD,), FILL, device=dev)
    t = buf[:numel].view(shape)
    if src is not None:
        t.copy_(src)
    return t, buf[numel:]


def run_entry(dev, spec, x0, v0, k, thin, h, *, gamma=GAMMA, temp=TEMP, noise=None, traj=True, seed=0, offset=0):
    """One call of the entry -> dict of CPU tensors x, v [n, dim], traj [n, k // thin, dim].  v0 None: draw_v0 = 1 and v starts
    from FILL.  Outputs start from FILL and sit in front of a guard: a slot the call did not write keeps it, and so must the guards."""
    n, dim = x0.shape
    model = model_of(spec, dev)
    x, gx = _guarded(dev, (n, dim), x0)
    v, gv = _guarded(dev, (n, dim), v0)
    tr, gt = _guarded(dev, (n, k // thin, dim)) if traj else (None, None)
    noise_d = None if noise is None else noise.to(dev).contiguous()
    before = hip_calls(ENTRY)
    _lib.call(ENTRY, model.fused_spec().to_c(), x.data_ptr(), v.data_ptr(), n, dim, k, h, gamma, temp, int(v0 is None), thin,
              _lib.ptr(tr), _lib.ptr(noise_d), seed, offset, _lib.stream_handle(dev))
    torch.cuda.synchronize()
    assert hip_calls(ENTRY) == before + 1
    for guard in (gx, gv, gt):
        assert guard is None or bool((guard == FILL).all()), "the call wrote behind an output"
    return {"x": x.cpu(), "v": v.cpu(), "traj": None if tr is None else tr.cpu()}


def _run_case(dev, c, **kw):
    return run_entry(dev, c["spec"], c["x0"], c["v0"], c["k"], c["thin"], c["h"], noise=c["noise"], **kw)


# ---------------------------------------------------------------------------------
# the recurrence, every kind
# ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind,dim,n,k,thin", EXACT_CASES)
def test_elementwise_cases_are_the_restatement_bit_for_bit(cuda_device, kind, dim, n, k, thin):
    c = case(kind, dim, n, k, thin)
    got = _run_case(cuda_device, c)
    ref = c["ref32"]
    assert torch.equal(got["x"], ref["x"]) and torch.equal(got["v"], ref["v"]) and torch.equal(got["traj"], ref["traj"])
    assert got["traj"].shape == (n, k // thin, dim) and not torch.equal(got["x"], c["x0"])


@gpu
@pytest.mark.parametrize("kind,dim,n,k,thin", COUPLED_CASES)
def test_coupled_cases_meet_the_yardstick(cuda_device, kind, dim, n, k, thin):
    c = case(kind, dim, n, k, thin)
    got = _run_case(cuda_device, c)
    ref32, ref64 = c["ref32"], c["ref64"]
    # the Langevin factor of test_tempering_gpu.py
    print(yardstick(got["x"], ref32["x"], ref64["x"], k_med=1.5, what=f"kinetic x {kind} dim {dim}"))
    print(yardstick(got["v"], ref32["v"], ref64["v"], k_med=1.5, what=f"kinetic v {kind} dim {dim}"))
    assert torch.isfinite(got["traj"]).all() and not bool((got["traj"] == FILL).any())
    if k % thin == 0:
        assert torch.equal(got["traj"][:, -1], got["x"])


# ---------------------------------------------------------------------------------
# native draws
# ---------------------------------------------------------------------------------
def _field(dev, seed, step, n_elem):
    out = torch.empty((n_elem + 3) // 4 * 4, device=dev)
    _lib.call("ebm_noise_fill_f32", out.data_ptr(), n_elem, _lib.NOISE_NORMAL, seed, step, _lib.stream_handle(dev))
    return out[:n_elem].clone()


@gpu
@pytest.mark.parametrize("kind,dim,n", [("double_well", 5, 37), ("harmonic", 100, 37), ("gmm", 32, 70), ("gaussian", 256, 9)])
def test_native_draws_are_the_materialised_fields(cuda_device, kind, dim, n):
    dev, (k, thin) = cuda_device, (11, 3)
    spec, h = energy_spec(kind, dim), STEP[kind]
    x0 = torch.randn(n, dim, generator=torch.Generator().manual_seed(5))
    seed, offset = 0x1234567887654321, 77
    sqrt_temp = constants(h, GAMMA, TEMP)[3]
    v0 = (sqrt_temp * _field(dev, seed, offset, n * dim)).view(n, dim).cpu()  # the start velocity: step `offset`
    noise = torch.stack([_field(dev, seed, offset + 1 + s, n * dim) for s in range(k)]).view(k, n, dim).cpu()
    native = run_entry(dev, spec, x0, None, k, thin, h, seed=seed, offset=offset)
    fed = run_entry(dev, spec, x0, v0, k, thin, h, noise=noise)
    for key in ("x", "v", "traj"):
        assert torch.equal(native[key], fed[key]), key
        assert torch.isfinite(native[key]).all()
    # injected noise with draw_v0: the start velocity still comes from the field
    mixed = run_entry(dev, spec, x0, None, k, thin, h, noise=noise, seed=seed, offset=offset)
    assert torch.equal(mixed["x"], fed["x"]) and torch.equal(mixed["v"], fed["v"])
    # a sub-block of chains run alone (another grid, other lanes) reproduces its rows of the full launch
    lo, hi = n // 3, n // 3 + max(n // 2, 1)
    part = run_entry(dev, spec, x0[lo:hi], v0[lo:hi], k, thin, h, noise=noise[:, lo:hi])
    for key in ("x", "v", "traj"):
        assert torch.equal(part[key], fed[key][lo:hi]), key


@gpu
@pytest.mark.parametrize("kind", ["double_well", "gaussian"])
@pytest.mark.parametrize("dim", [5, 100])
def test_two_calls_are_one(cuda_device, kind, dim):
    """(k1, offset) then (k2, offset + k1) with draw_v0 = 0 is one call of k1 + k2: kick and drift are not merged across steps."""
    dev, (n, k1, k2) = cuda_device, (37, 4, 7)
    spec, h = energy_spec(kind, dim), STEP[kind]
    x0 = torch.randn(n, dim, generator=torch.Generator().manual_seed(6))
    seed, offset = 0x0123456789ABCDEF, 41
    whole = run_entry(dev, spec, x0, None, k1 + k2, 1, h, seed=seed, offset=offset)
    first = run_entry(dev, spec, x0, None, k1, 1, h, seed=seed, offset=offset)
    second = run_entry(dev, spec, first["x"], first["v"], k2, 1, h, seed=seed, offset=offset + k1)
    assert torch.equal(second["x"], whole["x"]) and torch.equal(second["v"], whole["v"])
    assert torch.equal(torch.cat((first["traj"], second["traj"]), dim=1), whole["traj"])


# ---------------------------------------------------------------------------------
# what is written
# ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind,dim,n,k,thin", [("double_well", 5, 37, 11, 3), ("harmonic", 256, 257, 4, 2), ("gaussian", 100, 37, 1, 1),
                                               ("rosenbrock", 12, 37, 4, 2)])
def test_every_row_is_written_and_nothing_else(cuda_device, kind, dim, n, k, thin):
    c = case(kind, dim, n, k, thin)
    got = _run_case(cuda_device, c)  # (run_entry checks the guards behind x, v and traj)
    lean = _run_case(cuda_device, c, traj=False)
    assert lean["traj"] is None and torch.equal(lean["x"], got["x"]) and torch.equal(lean["v"], got["v"])
    for key in ("x", "v", "traj"):
        assert not bool((got[key] == FILL).any()), f"a slot of {key} was not written"
    # draw_v0: v is output only, every row written
    drawn = run_entry(cuda_device, c["spec"], c["x0"], None, k, thin, c["h"], noise=c["noise"], seed=3, offset=9)
    assert not bool((drawn["v"] == FILL).any()) and torch.isfinite(drawn["v"]).all()


# ---------------------------------------------------------------------------------
# non-finite inputs
# ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind,dim", [("double_well", 5), ("gaussian", 32)])
def test_wild_start_stays_in_its_chain(cuda_device, kind, dim):
    """A NaN coordinate in one chain and a 1e20 coordinate in another: every other chain's outputs are bitwise the clean run's."""
    n, k, thin = (37, 11, 3) if kind == "double_well" else (257, 4, 2)
    c = case(kind, dim, n, k, thin)
    x0 = c["x0"].clone()
    x0[3, 2] = float("nan")
    x0[7, 4] = 1e20
    got = run_entry(cuda_device, c["spec"], x0, c["v0"], k, thin, c["h"], noise=c["noise"])
    clean = _run_case(cuda_device, c)
    others = [i for i in range(n) if i not in (3, 7)]
    for key in ("x", "v", "traj"):
        assert torch.isfinite(clean[key]).all()
        assert torch.equal(got[key][others], clean[key][others]), key
    # (the wild chains did run wild: NaN spreads through a coupled row; 1e20 overflows the double well and stays huge on the Gaussian)
    assert torch.isnan(got["x"][3]).any() and not bool((got["x"][7].abs() < 1e10).all())


# ---------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------
@gpu
def test_refusals_launch_nothing(cuda_device):
    """The refusals of test_kinetic.py with real buffers: each raises its code and no buffer is touched."""
    from test_kinetic import REFUSALS, _abi_call

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
# through UnderdampedLangevin.sample()
# ---------------------------------------------------------------------------------
@gpu
def test_sample_is_one_launch(cuda_device):
    dev, (n, dim, k1, k2) = cuda_device, (300, 6, 17, 23)
    k = k1 + k2
    x0 = torch.randn(n, dim, device=dev)
    keep = x0.clone()
    spec = energy_spec("double_well", dim)
    s = ta.UnderdampedLangevin(model_of(spec, dev), step_size=0.05, friction=GAMMA, temperature=TEMP, device=dev)
    assert s._route(x0)[0] == "fused"
    g = torch.Generator(device=dev).manual_seed(5)
    before = dict(_lib.call_counts)
    x, v = s.sample(x=x0, n_steps=k, return_velocity=True, generator=g)
    torch.cuda.synchronize()
    new = {name: c - before.get(name, 0) for name, c in _lib.call_counts.items() if c != before.get(name, 0)}
    assert new == {ENTRY: 1}, new
    assert _rng._get_offset(g) == 4 * (k + 1)
    assert torch.equal(x0, keep), "the caller's tensor was touched"
    assert x.is_cuda and v.is_cuda and x.shape == v.shape == (n, dim) and torch.isfinite(x).all() and torch.isfinite(v).all()
    # the states are the entry's at the generator's coordinates
    want = run_entry(dev, spec, x0.cpu(), None, k, 1, 0.05, seed=_rng.kernel_seed(5), offset=0)
    assert torch.equal(x.cpu(), want["x"]) and torch.equal(v.cpu(), want["v"])
    # cut in two: the second call continues from the returned velocity at the Philox step the first one stopped at
    g = torch.Generator(device=dev).manual_seed(5)
    xa, va = s.sample(x=x0, n_steps=k1, return_velocity=True, generator=g)
    assert _rng._get_offset(g) == 4 * (k1 + 1)
    _rng._set_offset(g, 4 * k1)  # (a call owns k + 1 steps; the uncut run drew step k1 + 1 + s where this one draws its step 1 + s)
    va_keep = va.clone()
    xb, vb = s.sample(x=xa, n_steps=k2, velocity=va, return_velocity=True, reset_schedulers=False, generator=g)
    assert torch.equal(va, va_keep), "the caller's velocity was touched"
    assert torch.equal(xb, x) and torch.equal(vb, v)
    # trajectory and diagnostics: the kept positions and their statistics
    traj, diag = s.sample(x=x0, n_steps=k, thin=4, return_trajectory=True, return_diagnostics=True,
                          generator=torch.Generator(device=dev).manual_seed(5))
    assert traj.shape == (n, k // 4, dim) and torch.equal(traj[:, -1], x)
    assert torch.allclose(diag["mean"], traj.mean(dim=0), atol=1e-5)
    assert torch.allclose(diag["var"], traj.var(dim=0, unbiased=False), rtol=1e-4, atol=1e-6)
    assert torch.allclose(diag["energy"], torch.stack([s.model(traj[:, j].contiguous()).mean() for j in range(k // 4)]), rtol=1e-4)
    assert torch.allclose(diag["kinetic_temperature"], v.square().mean())


@gpu
def test_other_configurations_take_the_eager_route_on_the_gpu(cuda_device):
    dev = cuda_device
    before = hip_calls(ENTRY)
    sched = ta.UnderdampedLangevin(ta.HarmonicModel(k=4.0, device=dev), step_size=ta.core.schedules.LinearScheduler(0.3, 0.1, 10), device=dev)
    g = torch.Generator(device=dev).manual_seed(2)
    x = sched.sample(x=0.5 * torch.randn(2048, 2, device=dev), n_steps=30, generator=g)
    assert x.is_cuda and abs(x.var().item() * 4.0 - 1.0) < 0.15
    wide = ta.UnderdampedLangevin(ta.HarmonicModel(k=4.0, device=dev), step_size=0.3, device=dev)
    x = wide.sample(x=torch.zeros(8, 260, device=dev), n_steps=3, generator=g)
    assert x.shape == (8, 260) and torch.isfinite(x).all()
    assert hip_calls(ENTRY) == before


@gpu
def test_the_harmonic_law_holds_on_the_fused_route(cuda_device):
    from test_kinetic import LAW_SEED, check_harmonic_law, law_start

    dev, (n, dim) = cuda_device, (4096, 4)
    s = ta.UnderdampedLangevin(ta.HarmonicModel(k=4.0, device=dev), step_size=0.3, friction=1.0, temperature=1.0, device=dev)
    before = hip_calls(ENTRY)
    x, diag, v = s.sample(x=law_start(n, dim, 4.0, 1.0, LAW_SEED, dev), n_steps=400, return_diagnostics=True, return_velocity=True,
                          generator=torch.Generator(device=dev).manual_seed(LAW_SEED))
    assert hip_calls(ENTRY) == before + 1
    check_harmonic_law(x.cpu(), v.cpu(), {"kinetic_temperature": diag["kinetic_temperature"].cpu()}, 4.0, 1.0, 0.3)
    s2 = ta.UnderdampedLangevin(ta.HarmonicModel(k=1.0, device=dev), step_size=1.0, friction=0.5, temperature=2.0, device=dev)
    x, diag, v = s2.sample(x=law_start(n, dim, 1.0, 2.0, LAW_SEED, dev), n_steps=200, return_diagnostics=True, return_velocity=True,
                           generator=torch.Generator(device=dev).manual_seed(LAW_SEED))
    check_harmonic_law(x.cpu(), v.cpu(), {"kinetic_temperature": diag["kinetic_temperature"].cpu()}, 4.0 / 4.0, 2.0, 1.0)
