"""ebm_kinetic_mlp_chain_mass_f32 and ebm_ghmc_mlp_chain_mass_f32 on the GPU: the kernels through the C ABI with injected draws
against the restatements of mass_cases.py on the networks of mass_mlp_cases.py (the fp64 referee: the decisions equal, the states
within the fp32 restatement's own error), what they write and what they do not, mass 1 against the unit-mass MLP entries bit for
bit, their native draws against the materialised Philox fields, a run cut in two, a wild start, the refusals with real buffers,
sample() and ContrastiveDivergence with the opt-ins ``fused_mlp`` + ``fused_mlp_mass``, and the law of a confining 2-D network
with the mass (1, 4) against the CPU eager route."""

import copy
import math

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib, _rng
from helpers import hip_calls
import ghmc_mlp_cases
import kinetic_mlp_cases
import mass_cases
import mass_mlp_cases as mm
from mass_mlp_cases import GAMMA, TEMP
from torchebm_amd.utils.synthetic import two_moons

pytestmark = pytest.mark.gpu
BAOAB_ENTRY, GHMC_ENTRY = "ebm_kinetic_mlp_chain_mass_f32", "ebm_ghmc_mlp_chain_mass_f32"
BAOAB_UNIT, GHMC_UNIT = "ebm_kinetic_mlp_chain_f32", "ebm_ghmc_mlp_chain_f32"
FILL, MASK_FILL, MASS_FILL = 7.0, 9, 3.0
GUARD = 64  # elements behind every buffer that must keep their fill


def _guarded(dev, shape, src=None, dtype=torch.float32, fill=FILL):
    """A tensor of `shape` in front of GUARD elements of `fill` (in one allocation) -> (tensor, guard)."""
    numel = 1
    for s in shape:
        numel *= s
    buf = torch.full((numel + GUARD,), fill, device=dev, dtype=dtype)
    t = buf[:numel].view(shape)
    if src is not None:
        t.copy_(src)
    return t, buf[numel:]


def _mass_args(dev, mass):
    """(kind, scalar, diag tensor or None, its guard or None) of a mass as the entries take it; None: no mass arguments."""
    if isinstance(mass, float):
        return _lib.MASS_SCALAR, mass, None, None
    d, gd = _guarded(dev, tuple(mass.shape), mass, fill=MASS_FILL)
    return _lib.MASS_DIAG, 0.0, d, gd


def run_baoab(dev, cpu_model, x0, p0, k, thin, h, mass, *, noise=None, traj=True, seed=0, offset=0, gamma=GAMMA, temp=TEMP):
    """One call of the massed BAOAB entry (mass None: of the unit-mass MLP entry) -> dict of CPU tensors x, v, traj.  p0 None:
    draw_v0 = 1.  Outputs start from their fill in front of a guard; the diagonal sits in front of one too."""
    n, dim = x0.shape
    spec = copy.deepcopy(cpu_model).to(dev).fused_spec()
    x, gx = _guarded(dev, (n, dim), x0)
    v, gv = _guarded(dev, (n, dim), p0)
    tr, gt = _guarded(dev, (n, k // thin, dim)) if traj else (None, None)
    z_d = None if noise is None else noise.to(dev).contiguous()
    entry, m_args, gd = BAOAB_UNIT, (), None
    if mass is not None:
        kind, scalar, d, gd = _mass_args(dev, mass)
        entry, m_args = BAOAB_ENTRY, (kind, scalar, _lib.ptr(d))
    before = hip_calls(entry)
    _lib.call(entry, spec.to_c(), x.data_ptr(), v.data_ptr(), n, dim, k, h, gamma, temp, *m_args, int(p0 is None), thin, _lib.ptr(tr),
              _lib.ptr(z_d), seed, offset, _lib.stream_handle(dev))
    torch.cuda.synchronize()
    assert hip_calls(entry) == before + 1
    for guard, fill in ((gx, FILL), (gv, FILL), (gt, FILL), (gd, MASS_FILL)):
        assert guard is None or bool((guard == fill).all()), "the call wrote behind a buffer"
    return {"x": x.cpu(), "v": v.cpu(), "traj": None if tr is None else tr.cpu()}


def run_ghmc(dev, cpu_model, x0, p0, n_mh, thin, L, eps, mass, *, z=None, u=None, traj=True, mask=True, seed=0, offset=0, gamma=GAMMA,
             temp=TEMP):
    """One call of the massed GHMC entry (mass None: of the unit-mass MLP entry) -> x, v, traj, accepted."""
    n, dim = x0.shape
    spec = copy.deepcopy(cpu_model).to(dev).fused_spec()
    x, gx = _guarded(dev, (n, dim), x0)
    v, gv = _guarded(dev, (n, dim), p0)
    tr, gt = _guarded(dev, (n, n_mh // thin, dim)) if traj else (None, None)
    mk, gm = _guarded(dev, (n_mh, n), dtype=torch.uint8, fill=MASK_FILL) if mask else (None, None)
    z_d = None if z is None else z.to(dev).contiguous()
    u_d = None if u is None else u.to(dev).contiguous()
    entry, m_args, gd = GHMC_UNIT, (), None
    if mass is not None:
        kind, scalar, d, gd = _mass_args(dev, mass)
        entry, m_args = GHMC_ENTRY, (kind, scalar, _lib.ptr(d))
    before = hip_calls(entry)
    _lib.call(entry, spec.to_c(), x.data_ptr(), v.data_ptr(), n, dim, n_mh, L, eps, gamma, temp, *m_args, int(p0 is None), thin,
              _lib.ptr(tr), _lib.ptr(mk), _lib.ptr(z_d), _lib.ptr(u_d), seed, offset, _lib.stream_handle(dev))
    torch.cuda.synchronize()
    assert hip_calls(entry) == before + 1
    for guard, fill in ((gx, FILL), (gv, FILL), (gt, FILL), (gm, MASK_FILL), (gd, MASS_FILL)):
        assert guard is None or bool((guard == fill).all()), "the call wrote behind a buffer"
    if mk is not None:
        assert bool((mk <= 1).all()), "a slot of the accept mask was not written"
    return {"x": x.cpu(), "v": v.cpu(), "traj": None if tr is None else tr.cpu(), "accepted": None if mk is None else mk.cpu().bool()}


def _run_baoab_case(dev, c, **kw):
    return run_baoab(dev, c["cpu"], c["x0"], c["v0"], c["k"], c["thin"], c["h"], c["mass"], noise=c["noise"], **kw)


def _run_ghmc_case(dev, c, **kw):
    return run_ghmc(dev, c["cpu"], c["x0"], c["v0"], c["n_mh"], c["thin"], c["L"], c["eps"], c["mass"], z=c["z"], u=c["u"], **kw)


def _check_against_fp64(got, c, what):
    """x, v and the kept positions no further from fp64 than max(4 x the fp32 restatement's own max error, 4e-6 x max |ref|), the bar
    of test_kinetic_mlp_gpu.py and test_ghmc_mlp_gpu.py; every row written.  Every figure is printed in front of the assertions."""
    figures = {}
    for key in ("x", "v", "traj"):
        ref = c["ref64"][key]
        err_hip = (got[key].double() - ref).abs().max().item()
        err_torch = (c["ref32"][key].double() - ref).abs().max().item()
        figures[key] = (err_hip, err_torch, ref.abs().max().item())
        print(f"{what}: {key} kernel err {err_hip:.3e}, fp32 restatement err {err_torch:.3e} ({err_hip / max(err_torch, 1e-30):.2f} x), "
              f"max|ref| {figures[key][2]:.3e}")
    for key, (err_hip, err_torch, scale) in figures.items():
        assert not bool((got[key] == FILL).any()), f"a slot of {key} was not written"
        assert err_hip <= max(4.0 * err_torch, 4e-6 * scale), (key, err_hip, err_torch, scale)


# ---------------------------------------------------------------------------------
# the walks against the restatements
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("in_dim,hidden,n,k,thin,form", mm.BAOAB_CASES)
def test_baoab_cases_with_injected_noise(cuda_device, in_dim, hidden, n, k, thin, form):
    c = mm.baoab_case(in_dim, hidden, n, k, thin, form)
    got = _run_baoab_case(cuda_device, c)  # (run_baoab checks the guards behind x, p, traj and the diagonal)
    assert got["traj"].shape == (n, k // thin, in_dim)
    _check_against_fp64(got, c, f"BAOAB dim {in_dim} H {hidden} n {n} k {k} {form}")


@pytest.mark.parametrize("in_dim,hidden,n,n_mh,thin,L,form", mm.GHMC_CASES)
def test_ghmc_cases_with_injected_draws(cuda_device, in_dim, hidden, n, n_mh, thin, L, form):
    c = mm.ghmc_case(in_dim, hidden, n, n_mh, thin, L, form)
    got = _run_ghmc_case(cuda_device, c)
    assert got["traj"].shape == (n, n_mh // thin, in_dim) and got["accepted"].shape == (n_mh, n)
    wrong = int((got["accepted"] != c["ref64"]["accepted"]).sum())
    print(f"GHMC dim {in_dim} H {hidden} n {n} n_mh {n_mh} L {L} {form}: decisions that differ from fp64: {wrong} of {got['accepted'].numel()}")
    assert wrong == 0
    _check_against_fp64(got, c, f"GHMC dim {in_dim} H {hidden} n {n} n_mh {n_mh} L {L} {form}")


# ---------------------------------------------------------------------------------
# bit for bit
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("in_dim,hidden", mm.ANCHOR_SHAPES)
def test_baoab_with_mass_one_is_the_unit_mass_entry_bit_for_bit(cuda_device, in_dim, hidden):
    dev, (n, k, thin), cpu = cuda_device, (37, 4, 2), kinetic_mlp_cases.net(in_dim, hidden)
    x0, p0, noise, _ = mm.anchor_inputs(in_dim, n, k)
    h = 0.2
    want = run_baoab(dev, cpu, x0, p0, k, thin, h, None, noise=noise)
    drawn = run_baoab(dev, cpu, x0, None, k, thin, h, None, seed=5, offset=3)
    for mass in (1.0, torch.ones(in_dim)):
        got = run_baoab(dev, cpu, x0, p0, k, thin, h, mass, noise=noise)
        for key in ("x", "v", "traj"):
            assert torch.equal(got[key], want[key]), (key, type(mass))
        got = run_baoab(dev, cpu, x0, None, k, thin, h, mass, seed=5, offset=3)  # the start draw and the native noise too
        for key in ("x", "v", "traj"):
            assert torch.equal(got[key], drawn[key]), (key, type(mass))
    assert not torch.equal(want["x"], x0) and torch.isfinite(want["x"]).all()
    other = run_baoab(dev, cpu, x0, p0, k, thin, h, 0.37, noise=noise)  # (the mass is read)
    assert not torch.equal(other["x"], want["x"])


@pytest.mark.parametrize("in_dim,hidden", mm.ANCHOR_SHAPES)
def test_ghmc_with_mass_one_is_the_unit_mass_entry_bit_for_bit(cuda_device, in_dim, hidden):
    dev, (n, n_mh, thin, L), cpu = cuda_device, (37, 4, 2, 2), ghmc_mlp_cases.net(in_dim, hidden)
    x0, p0, z, u = mm.anchor_inputs(in_dim, n, n_mh)
    eps = 1.0
    want = run_ghmc(dev, cpu, x0, p0, n_mh, thin, L, eps, None, z=z, u=u)
    drawn = run_ghmc(dev, cpu, x0, None, n_mh, thin, L, eps, None, seed=5, offset=3)
    for mass in (1.0, torch.ones(in_dim)):
        got = run_ghmc(dev, cpu, x0, p0, n_mh, thin, L, eps, mass, z=z, u=u)
        for key in ("x", "v", "traj", "accepted"):
            assert torch.equal(got[key], want[key]), (key, type(mass))
        got = run_ghmc(dev, cpu, x0, None, n_mh, thin, L, eps, mass, seed=5, offset=3)
        for key in ("x", "v", "traj", "accepted"):
            assert torch.equal(got[key], drawn[key]), (key, type(mass))
    assert want["accepted"].any() and (~want["accepted"]).any()  # both branches ran
    other = run_ghmc(dev, cpu, x0, p0, n_mh, thin, L, eps, 0.37, z=z, u=u)
    assert not torch.equal(other["v"], want["v"])


def _field(dev, kind, seed, step, n_elem):
    out = torch.empty((n_elem + 3) // 4 * 4, device=dev)
    _lib.call("ebm_noise_fill_f32", out.data_ptr(), n_elem, kind, seed, step, _lib.stream_handle(dev))
    return out[:n_elem].clone()


def _start_momentum(dev, mass, seed, offset, n, dim):
    """(sqrt_temp m_sqrt) z0, z0 the normal field at step `offset`, in fp32 as the kernel forms it."""
    sqrt_temp = torch.tensor(math.sqrt(TEMP), dtype=torch.float64).float()
    m_sqrt = mass_cases.forms(mass, torch.float32)[1]
    return (sqrt_temp * m_sqrt) * _field(dev, _lib.NOISE_NORMAL, seed, offset, n * dim).view(n, dim).cpu()


@pytest.mark.parametrize("form", ["scalar", "diag"])
@pytest.mark.parametrize("in_dim,hidden", mm.PHILOX_DIMS)
def test_baoab_native_draws_are_the_materialised_fields(cuda_device, in_dim, hidden, form):
    dev, (n, k, thin), cpu = cuda_device, (70, 5, 2), kinetic_mlp_cases.net(in_dim, hidden)
    mass = mm.mass_of(form, in_dim)
    h = mm.baoab_step(mass)
    x0 = torch.randn(n, in_dim, generator=torch.Generator().manual_seed(5))
    seed, offset = 0x1234567887654321, 77
    p0 = _start_momentum(dev, mass, seed, offset, n, in_dim)
    noise = torch.stack([_field(dev, _lib.NOISE_NORMAL, seed, offset + 1 + i, n * in_dim) for i in range(k)]).view(k, n, in_dim).cpu()
    native = run_baoab(dev, cpu, x0, None, k, thin, h, mass, seed=seed, offset=offset)
    fed = run_baoab(dev, cpu, x0, p0, k, thin, h, mass, noise=noise)
    for key in ("x", "v", "traj"):
        assert torch.equal(native[key], fed[key]), key
        assert torch.isfinite(native[key]).all() and not bool((native[key] == FILL).any())
    mixed = run_baoab(dev, cpu, x0, None, k, thin, h, mass, noise=noise, seed=seed, offset=offset)  # injected noise with draw_v0
    assert torch.equal(mixed["x"], fed["x"]) and torch.equal(mixed["v"], fed["v"])
    lean = run_baoab(dev, cpu, x0, p0, k, thin, h, mass, noise=noise, traj=False)  # a call without traj: the same x and p
    assert lean["traj"] is None and torch.equal(lean["x"], fed["x"]) and torch.equal(lean["v"], fed["v"])
    # two calls equal one
    k1 = 2
    first = run_baoab(dev, cpu, x0, None, k1, 1, h, mass, seed=seed, offset=offset)
    second = run_baoab(dev, cpu, first["x"], first["v"], k - k1, 1, h, mass, seed=seed, offset=offset + k1)
    assert torch.equal(second["x"], native["x"]) and torch.equal(second["v"], native["v"])


@pytest.mark.parametrize("form", ["scalar", "diag"])
@pytest.mark.parametrize("in_dim,hidden", mm.PHILOX_DIMS)
def test_ghmc_native_draws_are_the_materialised_fields(cuda_device, in_dim, hidden, form):
    dev, (n, n_mh, thin, L), cpu = cuda_device, (70, 5, 2, 2), ghmc_mlp_cases.net(in_dim, hidden)
    mass = mm.mass_of(form, in_dim)
    eps = mm.ghmc_step(mass)
    x0 = torch.randn(n, in_dim, generator=torch.Generator().manual_seed(5))
    seed, offset = 0x1234567887654321, 77
    p0 = _start_momentum(dev, mass, seed, offset, n, in_dim)
    z = torch.stack([_field(dev, _lib.NOISE_NORMAL, seed, offset + 1 + 2 * t, n * in_dim) for t in range(n_mh)]).view(n_mh, n, in_dim).cpu()
    u = torch.stack([_field(dev, _lib.NOISE_UNIFORM, seed, offset + 2 + 2 * t, n) for t in range(n_mh)]).view(n_mh, n).cpu()
    native = run_ghmc(dev, cpu, x0, None, n_mh, thin, L, eps, mass, seed=seed, offset=offset)
    fed = run_ghmc(dev, cpu, x0, p0, n_mh, thin, L, eps, mass, z=z, u=u)
    keys = ("x", "v", "traj", "accepted")
    for key in keys:
        assert torch.equal(native[key], fed[key]), key
    assert all(torch.isfinite(native[key]).all() for key in ("x", "v", "traj"))
    assert native["accepted"].any() and (~native["accepted"]).any()  # both branches ran
    for kw in (dict(z=z), dict(u=u)):  # either draw injected without the other
        mixed = run_ghmc(dev, cpu, x0, None, n_mh, thin, L, eps, mass, seed=seed, offset=offset, **kw)
        for key in keys:
            assert torch.equal(mixed[key], fed[key]), (key, sorted(kw))
    lean = run_ghmc(dev, cpu, x0, p0, n_mh, thin, L, eps, mass, z=z, u=u, traj=False, mask=False)
    assert lean["traj"] is None and lean["accepted"] is None and torch.equal(lean["x"], fed["x"]) and torch.equal(lean["v"], fed["v"])
    # two calls equal one
    n1 = 2
    whole = run_ghmc(dev, cpu, x0, None, n_mh, 1, L, eps, mass, seed=seed, offset=offset)
    first = run_ghmc(dev, cpu, x0, None, n1, 1, L, eps, mass, seed=seed, offset=offset)
    second = run_ghmc(dev, cpu, first["x"], first["v"], n_mh - n1, 1, L, eps, mass, seed=seed, offset=offset + 2 * n1)
    assert torch.equal(second["x"], whole["x"]) and torch.equal(second["v"], whole["v"])
    assert torch.equal(torch.cat((first["accepted"], second["accepted"])), whole["accepted"])
    assert torch.equal(torch.cat((first["traj"], second["traj"]), dim=1), whole["traj"])


# ---------------------------------------------------------------------------------
# non-finite inputs
# ---------------------------------------------------------------------------------
def _wild(x0):
    x0 = x0.clone()
    x0[3, 2] = float("nan")
    x0[7, 4] = 1e20
    return x0


@pytest.mark.parametrize("in_dim,hidden,n,k,thin,form", [(5, 128, 37, 4, 2, "diag"), (40, 64, 37, 4, 2, "scalar")])
def test_a_wild_start_stays_in_its_chain_under_baoab(cuda_device, in_dim, hidden, n, k, thin, form):
    c = mm.baoab_case(in_dim, hidden, n, k, thin, form)
    got = run_baoab(cuda_device, c["cpu"], _wild(c["x0"]), c["v0"], k, thin, c["h"], c["mass"], noise=c["noise"])
    clean = _run_baoab_case(cuda_device, c)
    others = [i for i in range(n) if i not in (3, 7)]
    for key in ("x", "v", "traj"):
        assert torch.isfinite(clean[key]).all() and torch.equal(got[key][others], clean[key][others]), key


@pytest.mark.parametrize("in_dim,hidden,n,n_mh,thin,L,form", [(5, 128, 37, 4, 2, 1, "diag"), (33, 128, 37, 4, 2, 3, "diag"),
                                                              (40, 64, 37, 4, 2, 1, "scalar")])
def test_a_wild_start_stays_in_its_chain_under_ghmc(cuda_device, in_dim, hidden, n, n_mh, thin, L, form):
    """A NaN and a 1e20 coordinate in the first wave (which then takes the literal path of the trajectory): every other chain's
    outputs are bitwise the clean run's."""
    c = mm.ghmc_case(in_dim, hidden, n, n_mh, thin, L, form)
    got = run_ghmc(cuda_device, c["cpu"], _wild(c["x0"]), c["v0"], n_mh, thin, L, c["eps"], c["mass"], z=c["z"], u=c["u"])
    clean = _run_ghmc_case(cuda_device, c)
    others = [i for i in range(n) if i not in (3, 7)]
    for key in ("x", "v", "traj"):
        assert torch.isfinite(clean[key]).all() and torch.equal(got[key][others], clean[key][others]), key
    assert torch.equal(got["accepted"][:, others], clean["accepted"][:, others])
    assert torch.equal(clean["accepted"], c["ref64"]["accepted"])


# ---------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("baoab", [True, False], ids=["baoab", "ghmc"])
def test_refusals_launch_nothing(cuda_device, baoab):
    """The refusals of test_mass_mlp.py with real buffers: each raises its code and no buffer is touched, the diagonal's included."""
    from test_mass_mlp import MASS_REFUSALS, _unit_refusals, baoab_abi_call, ghmc_abi_call

    call = baoab_abi_call if baoab else ghmc_abi_call
    dev, (n, dim) = cuda_device, (4, 8)
    x = torch.full((n, 132), FILL, device=dev)
    v = torch.full((n, 132), FILL, device=dev)
    d = torch.full((132,), MASS_FILL, device=dev)
    real = dict(x=x.data_ptr(), v=v.data_ptr())
    desc = ta.MLPEnergy(dim, 64, device=dev).fused_spec().to_c()
    for kw, match in _unit_refusals(baoab) + MASS_REFUSALS:
        with pytest.raises(ValueError, match=match):
            call(desc, **{**real, **kw})
    for kw, match in _unit_refusals(baoab):  # ... with a diagonal at hand
        with pytest.raises(ValueError, match=match):
            call(desc, **{**real, "mass_kind": _lib.MASS_DIAG, "diag": d.data_ptr(), **kw})
    with pytest.raises(ValueError, match="bad shape"):
        call(desc, n=-1, **real)
    with pytest.raises(ValueError, match="16-byte aligned"):
        call(desc, **{**real, "v": v.data_ptr() + 4})
    with pytest.raises(ValueError, match="energy descriptor is NULL"):
        call(None, **real)
    with pytest.raises(RuntimeError, match=r"code -2.*MLP energy only"):
        call(ta.DoubleWellModel(device=dev).fused_spec().to_c(), **real)
    with pytest.raises(RuntimeError, match=r"code -2.*MLP energy only"):
        call(ta.GaussianModel(torch.zeros(dim), torch.eye(dim), device=dev).fused_spec().to_c(), mass_kind=_lib.MASS_DIAG, diag=d.data_ptr(), **real)
    with pytest.raises(RuntimeError, match=r"code -3.*got 64, 129"):
        call(desc, dim=129, mass_kind=_lib.MASS_DIAG, diag=d.data_ptr(), **real)
    with pytest.raises(RuntimeError, match=r"code -3.*got 64, 0"):
        call(desc, dim=0, **real)
    wide = ta.MLPEnergy(dim, 64, device=dev).fused_spec().to_c()
    wide.n_comp = 96
    with pytest.raises(RuntimeError, match=r"code -3.*got 96, 8"):
        call(wide, **real)
    torch.cuda.synchronize()
    assert bool((x == FILL).all()) and bool((v == FILL).all()) and bool((d == MASS_FILL).all())


# ---------------------------------------------------------------------------------
# through sample()
# ---------------------------------------------------------------------------------
def _sampler(cls, model, step, mass, dev, **kw):
    extra = dict(n_leapfrog_steps=2) if cls is ta.GeneralizedHMC else {}
    return cls(model, step_size=step, friction=GAMMA, temperature=TEMP, mass=mass, device=dev, **extra, **kw)


@pytest.mark.parametrize("form", ["scalar", "diag"])
@pytest.mark.parametrize("cls", [ta.UnderdampedLangevin, ta.GeneralizedHMC], ids=["baoab", "ghmc"])
def test_sample_with_the_opt_ins_is_one_launch(cuda_device, cls, form):
    baoab = cls is ta.UnderdampedLangevin
    entry, per_step = (BAOAB_ENTRY, 1) if baoab else (GHMC_ENTRY, 2)
    dev, (n, dim, k1, k2) = cuda_device, (300, 6, 3, 5)
    k = k1 + k2
    cpu = (kinetic_mlp_cases.net if baoab else ghmc_mlp_cases.net)(dim, 64)
    mass = mm.mass_of(form, dim)
    step = mm.baoab_step(mass) if baoab else mm.ghmc_step(mass)
    model = copy.deepcopy(cpu).to(dev)
    x0 = torch.randn(n, dim, device=dev)
    keep = x0.clone()
    s = _sampler(cls, model, step, mass, dev)
    assert s._route(x0)[0] == "eager"
    s.fused_mlp = True
    assert s._route(x0)[0] == "eager"  # fused_mlp alone
    s.fused_mlp_mass = True
    assert s._route(x0)[0] == "fused_mlp_mass"
    g = torch.Generator(device=dev).manual_seed(5)
    before = hip_calls(entry)
    x, p = s.sample(x=x0, n_steps=k, return_velocity=True, generator=g)
    torch.cuda.synchronize()
    assert hip_calls(entry) == before + 1
    assert _rng._get_offset(g) == 4 * (per_step * k + 1)  # the steps the unit-mass MLP route reserves
    assert torch.equal(x0, keep), "the caller's tensor was touched"
    # the states are the entry's at the generator's coordinates
    if baoab:
        want = run_baoab(dev, cpu, x0.cpu(), None, k, 1, step, mass, seed=_rng.kernel_seed(5), offset=0)
    else:
        want = run_ghmc(dev, cpu, x0.cpu(), None, k, 1, 2, step, mass, seed=_rng.kernel_seed(5), offset=0)
        assert want["accepted"].any()
    assert torch.equal(x.cpu(), want["x"]) and torch.equal(p.cpu(), want["v"])
    # cut in two: the second call continues from the returned momentum at the Philox step the first one stopped at
    g = torch.Generator(device=dev).manual_seed(5)
    xa, pa = s.sample(x=x0, n_steps=k1, return_velocity=True, generator=g)
    _rng._set_offset(g, 4 * per_step * k1)
    pa_keep = pa.clone()
    xb, pb = s.sample(x=xa, n_steps=k2, velocity=pa, return_velocity=True, reset_schedulers=False, generator=g)
    assert torch.equal(pa, pa_keep), "the caller's momentum was touched"
    assert torch.equal(xb, x) and torch.equal(pb, p)
    # diagnostics: kinetic_temperature of p^2 / m, GHMC's acceptance from the mask
    traj, diag = s.sample(x=x0, n_steps=k, thin=4, return_trajectory=True, return_diagnostics=True,
                          generator=torch.Generator(device=dev).manual_seed(5))
    assert traj.shape == (n, k // 4, dim) and torch.equal(traj[:, -1].cpu(), want["traj"][:, 3::4][:, -1])
    m = mass if form == "scalar" else mass.to(dev)
    assert torch.allclose(diag["kinetic_temperature"], (p.square() / m).mean())
    if not baoab:
        want_rate = want["accepted"][3::4][: k // 4].float().mean(dim=1)
        assert torch.allclose(diag["acceptance_rate"].cpu(), want_rate, rtol=1e-6, atol=0)
    # no step: no launch of the entry, the start momentum from the field
    before = hip_calls(entry)
    x, p = s.sample(x=x0, n_steps=0, return_velocity=True, generator=torch.Generator(device=dev).manual_seed(5))
    assert hip_calls(entry) == before and torch.equal(x, x0) and x.data_ptr() != x0.data_ptr()
    assert torch.equal(p.cpu(), _start_momentum(dev, mass, _rng.kernel_seed(5), 0, n, dim))


@pytest.mark.parametrize("cls", [ta.UnderdampedLangevin, ta.GeneralizedHMC], ids=["baoab", "ghmc"])
def test_without_the_second_opt_in_and_off_the_shapes_sample_stays_eager(cuda_device, cls):
    dev = cuda_device
    entry = BAOAB_ENTRY if cls is ta.UnderdampedLangevin else GHMC_ENTRY
    before = hip_calls(entry)
    torch.manual_seed(3)
    mass = mm.mass_of("diag", 6).to(dev)
    s = _sampler(cls, ta.MLPEnergy(6, 64, device=dev), 0.1, mass, dev)
    s.fused_mlp = True
    x0 = torch.randn(64, 6, device=dev)
    assert s._route(x0)[0] == "eager"
    out = s.sample(x=x0, n_steps=3, generator=torch.Generator(device=dev).manual_seed(1))
    assert out.shape == (64, 6) and out.is_cuda and torch.isfinite(out).all()
    s.fused_mlp_mass = True
    assert s._route(x0)[0] == "fused_mlp_mass" and s._route(torch.zeros(4, 7, device=dev))[0] == "eager"
    assert s._route(x0, {"label": 1})[0] == "eager" and s._route(x0.double())[0] == "eager"
    odd = _sampler(cls, ta.MLPEnergy(8, 96, device=dev), 0.1, 0.37, dev)
    odd.fused_mlp = odd.fused_mlp_mass = True
    assert odd._route(torch.zeros(4, 8, device=dev))[0] == "eager"
    sched = cls(ta.MLPEnergy(6, 64, device=dev), step_size=ta.core.schedules.LinearScheduler(0.3, 0.1, 10), mass=0.37, device=dev)
    sched.fused_mlp = sched.fused_mlp_mass = True
    assert sched._route(x0)[0] == "eager"
    assert hip_calls(entry) == before


@pytest.mark.parametrize("persistent", [False, True], ids=["cd_k", "persistent"])
@pytest.mark.parametrize("cls", [ta.UnderdampedLangevin, ta.GeneralizedHMC], ids=["baoab", "ghmc"])
def test_contrastive_divergence_makes_one_launch_per_call(cuda_device, cls, persistent):
    dev = cuda_device
    entry = BAOAB_ENTRY if cls is ta.UnderdampedLangevin else GHMC_ENTRY
    torch.manual_seed(6)
    model = ta.MLPEnergy(2, 64, device=dev)
    sampler = _sampler(cls, model, 0.1, torch.tensor([1.0, 4.0]), dev)
    sampler.fused_mlp = sampler.fused_mlp_mass = True
    cd = ta.losses.ContrastiveDivergence(model=model, sampler=sampler, k_steps=5, persistent=persistent, buffer_size=512, init_steps=0,
                                         device=dev)
    data = two_moons(n_samples=256, noise=0.05, seed=0, device=dev)
    g = torch.Generator(device=dev).manual_seed(7)
    for _ in range(3):
        before = hip_calls(entry)
        model.zero_grad()
        loss, negatives = cd(data, generator=g)
        assert hip_calls(entry) == before + 1
        assert torch.isfinite(loss) and negatives.shape == data.shape and negatives.is_cuda and torch.isfinite(negatives).all()
        loss.backward()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())


# ---------------------------------------------------------------------------------
# the law
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [ta.UnderdampedLangevin, ta.GeneralizedHMC], ids=["baoab", "ghmc"])
def test_the_law_of_a_confining_network_with_a_mass_is_the_eager_routes(cuda_device, cls):
    """The confining 2-D network of test_ais_mlp_gpu.py, mass (1, 4), n = 4096, 300 steps, seed 0, the step sizes and gamma, T of the
    unit-mass MLP law tests (h = 0.3; eps = 0.3, L = 2; gamma = 1, T = 1), on the fused massed route and on the CPU eager massed
    route: the mean energy of the final positions and the kinetic temperature (of p^2 / m) differ by at most 4.5 standard errors
    of the difference, taken from the chains' sample variances."""
    from test_ais_mlp_gpu import _confining_net

    baoab = cls is ta.UnderdampedLangevin
    entry = BAOAB_ENTRY if baoab else GHMC_ENTRY
    cpu = _confining_net()
    referee = copy.deepcopy(cpu).double()
    n, dim, k = 4096, 2, 300
    mass = torch.tensor([1.0, 4.0])
    x0 = torch.randn(n, dim, generator=torch.Generator().manual_seed(0))
    stats = {}
    for dev in (cuda_device, torch.device("cpu")):
        model = copy.deepcopy(cpu).to(dev)
        extra = {} if baoab else dict(n_leapfrog_steps=2)
        s = cls(model, step_size=0.3, friction=1.0, temperature=1.0, mass=mass, device=dev, **extra)
        s.fused_mlp = s.fused_mlp_mass = True
        assert s._route(x0.to(dev))[0] == ("fused_mlp_mass" if dev.type == "cuda" else "eager")
        before = hip_calls(entry)
        x, diag, p = s.sample(x=x0.to(dev), n_steps=k, return_diagnostics=True, return_velocity=True,
                              generator=torch.Generator(device=dev).manual_seed(0))
        assert hip_calls(entry) == before + (1 if dev.type == "cuda" else 0)
        with torch.no_grad():
            e = referee(x.cpu().double())
        kt = (p.cpu().double().square() / mass.double()).mean(dim=1)
        assert torch.isfinite(e).all() and torch.isfinite(kt).all()
        assert math.isclose(kt.mean().item(), diag["kinetic_temperature"].item(), rel_tol=1e-5)
        stats[dev.type] = {"e": (e.mean().item(), e.std().item() / math.sqrt(n)), "kt": (kt.mean().item(), kt.std().item() / math.sqrt(n))}
        if not baoab:
            rate = diag["acceptance_rate"].double().mean().item()
            print(f"{dev.type}: acceptance {rate:.4f}")
            assert 0.0 < rate < 1.0
    for key in ("e", "kt"):
        (m1, se1), (m2, se2) = stats["cuda"][key], stats["cpu"][key]
        z = (m1 - m2) / math.sqrt(se1**2 + se2**2)
        print(f"{key}: fused massed route {m1:.4f} +- {se1:.4f}, CPU eager massed route {m2:.4f} +- {se2:.4f}, z = {z:+.2f}")
    for key in ("e", "kt"):
        (m1, se1), (m2, se2) = stats["cuda"][key], stats["cpu"][key]
        assert abs(m1 - m2) <= 4.5 * math.sqrt(se1**2 + se2**2), (key, stats)
