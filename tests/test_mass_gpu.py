"""ebm_kinetic_chain_mass_f32 and ebm_ghmc_chain_mass_f32 on the GPU: both recurrences against the restatements of mass_cases.py,
mass 1 against the unit-mass entries and gamma = inf against ebm_hmc_chain_f32 with the same mass (bit for bit), the native
draws against the materialised Philox fields, a run cut in two, what is written and what is not, non-finite inputs, the
refusals, the two samplers on top of the entries, and both laws on the fused route."""

import math

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib, _rng
from helpers import hip_calls, yardstick
import mass_cases as mc
from mass_cases import GAMMA, TEMP, energy_spec, model_of

gpu = pytest.mark.gpu
BAOAB_ENTRY, GHMC_ENTRY = "ebm_kinetic_chain_mass_f32", "ebm_ghmc_chain_mass_f32"
FILL = 7.0
GUARD = 64  # elements behind every buffer that must keep FILL
FORMS = ("scalar", "diag")


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


def _mass_on(dev, mass, dim):
    """(kind, scalar, pointer), the diagonal's device tensor (kept alive by the caller) and its guard."""
    if isinstance(mass, float):
        return (_lib.MASS_SCALAR, mass, None), None, None
    m, gm = _guarded(dev, (dim,), mass)
    return (_lib.MASS_DIAG, 0.0, m.data_ptr()), m, gm


def run_baoab(dev, spec, mass, x0, p0, k, thin, h, *, gamma=GAMMA, temp=TEMP, noise=None, traj=True, seed=0, offset=0):
    """One call of the massed BAOAB entry -> dict of CPU tensors x, v (the momentum) [n, dim], traj [n, k // thin, dim].  p0 None:
    draw_v0 = 1 and the plane starts from FILL.  Outputs start from FILL and sit in front of a guard, as the mass does."""
    n, dim = x0.shape
    x, gx = _guarded(dev, (n, dim), x0)
    v, gv = _guarded(dev, (n, dim), p0)
    tr, gt = _guarded(dev, (n, k // thin, dim)) if traj else (None, None)
    noise_d = None if noise is None else noise.to(dev).contiguous()
    m_args, m_dev, gm = _mass_on(dev, mass, dim)
    before = hip_calls(BAOAB_ENTRY)
    _lib.call(BAOAB_ENTRY, model_of(spec, dev).fused_spec().to_c(), x.data_ptr(), v.data_ptr(), n, dim, k, h, gamma, temp, *m_args,
              int(p0 is None), thin, _lib.ptr(tr), _lib.ptr(noise_d), seed, offset, _lib.stream_handle(dev))
    torch.cuda.synchronize()
    assert hip_calls(BAOAB_ENTRY) == before + 1
    for guard in (gx, gv, gt, gm):
        assert guard is None or bool((guard == FILL).all()), "the call wrote behind a buffer"
    assert m_dev is None or torch.equal(m_dev.cpu(), mass), "the mass was written"
    return {"x": x.cpu(), "v": v.cpu(), "traj": None if tr is None else tr.cpu()}


def run_ghmc(dev, spec, mass, x0, p0, n_mh, thin, L, eps, *, gamma=GAMMA, temp=TEMP, z=None, u=None, traj=True, mask=True, seed=0,
             offset=0):
    """One call of the massed generalized-HMC entry -> dict of CPU tensors x, v (the momentum), traj, accepted [n_mh, n]."""
    n, dim = x0.shape
    x, gx = _guarded(dev, (n, dim), x0)
    v, gv = _guarded(dev, (n, dim), p0)
    tr, gt = _guarded(dev, (n, n_mh // thin, dim)) if traj else (None, None)
    mk, gk = _guarded(dev, (n_mh, n), dtype=torch.uint8) if mask else (None, None)
    z_d = None if z is None else z.to(dev).contiguous()
    u_d = None if u is None else u.to(dev).contiguous()
    m_args, m_dev, gm = _mass_on(dev, mass, dim)
    before = hip_calls(GHMC_ENTRY)
    _lib.call(GHMC_ENTRY, model_of(spec, dev).fused_spec().to_c(), x.data_ptr(), v.data_ptr(), n, dim, n_mh, L, eps, gamma, temp, *m_args,
              int(p0 is None), thin, _lib.ptr(tr), _lib.ptr(mk), _lib.ptr(z_d), _lib.ptr(u_d), seed, offset, _lib.stream_handle(dev))
    torch.cuda.synchronize()
    assert hip_calls(GHMC_ENTRY) == before + 1
    for guard in (gx, gv, gt, gk, gm):
        assert guard is None or bool((guard == FILL).all()), "the call wrote behind a buffer"
    assert m_dev is None or torch.equal(m_dev.cpu(), mass), "the mass was written"
    out = {"x": x.cpu(), "v": v.cpu(), "traj": None if tr is None else tr.cpu(), "accepted": None}
    if mask:
        mk = mk.cpu()
        assert int(mk.max()) <= 1, "a row of the accept mask was not written"
        out["accepted"] = mk.bool()
    return out


def _run_baoab_case(dev, c, **kw):
    return run_baoab(dev, c["spec"], c["mass"], c["x0"], c["v0"], c["k"], c["thin"], c["h"], noise=c["noise"], **kw)


def _run_ghmc_case(dev, c, **kw):
    return run_ghmc(dev, c["spec"], c["mass"], c["x0"], c["v0"], c["n_mh"], c["thin"], c["L"], c["eps"], gamma=c["gamma"], temp=c["temp"],
                    z=c["z"], u=c["u"], **kw)


# ---------------------------------------------------------------------------------
# against the restatements
# ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind,dim,n,k,thin,form", mc.BAOAB_EXACT)
def test_elementwise_baoab_cases_are_the_restatement_bit_for_bit(cuda_device, kind, dim, n, k, thin, form):
    c = mc.baoab_case(kind, dim, n, k, thin, form)
    got, ref = _run_baoab_case(cuda_device, c), c["ref32"]
    assert torch.equal(got["x"], ref["x"]) and torch.equal(got["v"], ref["v"]) and torch.equal(got["traj"], ref["traj"])
    assert got["traj"].shape == (n, k // thin, dim) and not torch.equal(got["x"], c["x0"])


@gpu
@pytest.mark.parametrize("kind,dim,n,k,thin,form", mc.BAOAB_COUPLED)
def test_coupled_baoab_cases_meet_the_yardstick(cuda_device, kind, dim, n, k, thin, form):
    c = mc.baoab_case(kind, dim, n, k, thin, form)
    got, ref32, ref64 = _run_baoab_case(cuda_device, c), c["ref32"], c["ref64"]
    # the factor test_kinetic_gpu.py gives the same code at unit mass
    print(yardstick(got["x"], ref32["x"], ref64["x"], k_med=1.5, what=f"baoab x {kind} dim {dim} {form}"))
    print(yardstick(got["v"], ref32["v"], ref64["v"], k_med=1.5, what=f"baoab p {kind} dim {dim} {form}"))
    assert torch.isfinite(got["traj"]).all() and not bool((got["traj"] == FILL).any())
    if k % thin == 0:
        assert torch.equal(got["traj"][:, -1], got["x"])


@gpu
@pytest.mark.parametrize("kind,dim,n,n_mh,thin,L,form", mc.GHMC_CASES)
def test_ghmc_cases_with_injected_draws(cuda_device, kind, dim, n, n_mh, thin, L, form):
    c = mc.ghmc_case(kind, dim, n, n_mh, thin, L, form)
    assert c["found"]
    ref32, ref64 = c["ref32"], c["ref64"]
    got = _run_ghmc_case(cuda_device, c)
    assert torch.equal(got["accepted"], ref32["accepted"])
    assert got["traj"].shape == (n, n_mh // thin, dim) and not bool((got["traj"] == FILL).any())
    rows = lambda t: t.reshape(-1, dim)  # noqa: E731
    # the factor test_ghmc_gpu.py gives the same trajectory code at unit mass
    print(yardstick(got["x"], ref32["x"], ref64["x"], k_med=2.0, what=f"ghmc x {kind} dim {dim} {form}"))
    print(yardstick(got["v"], ref32["v"], ref64["v"], k_med=2.0, what=f"ghmc p {kind} dim {dim} {form}"))
    print(yardstick(rows(got["traj"]), rows(ref32["traj"]), rows(ref64["traj"]), k_med=2.0, what=f"ghmc traj {kind} dim {dim} {form}"))
    if n_mh % thin == 0:
        assert torch.equal(got["traj"][:, -1], got["x"])


# ---------------------------------------------------------------------------------
# against the existing entries
# ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", ["double_well", "gmm"])
@pytest.mark.parametrize("dim", [5, 100])
def test_baoab_at_mass_one_is_the_unit_mass_entry(cuda_device, kind, dim):
    from test_kinetic_gpu import run_entry

    dev, (n, k, thin) = cuda_device, (37, 11, 3)
    spec, h = energy_spec(kind, dim), mc.kinetic_cases.STEP[kind]
    g = torch.Generator().manual_seed(41)
    x0, v0, noise = torch.randn(n, dim, generator=g), torch.randn(n, dim, generator=g), torch.randn(k, n, dim, generator=g)
    want = run_entry(dev, spec, x0, v0, k, thin, h, noise=noise)
    want_drawn = run_entry(dev, spec, x0, None, k, thin, h, seed=9, offset=5)
    for mass in (1.0, torch.ones(dim)):
        got = run_baoab(dev, spec, mass, x0, v0, k, thin, h, noise=noise)
        drawn = run_baoab(dev, spec, mass, x0, None, k, thin, h, seed=9, offset=5)
        for key in ("x", "v", "traj"):
            assert torch.equal(got[key], want[key]) and torch.equal(drawn[key], want_drawn[key]), key
    assert not torch.equal(want["x"], x0)


@gpu
@pytest.mark.parametrize("kind", ["double_well", "gmm"])
@pytest.mark.parametrize("dim", [5, 100])
def test_ghmc_at_mass_one_is_the_unit_mass_entry(cuda_device, kind, dim):
    from test_ghmc_gpu import run_entry

    dev, (n, n_mh, thin, L) = cuda_device, (37, 7, 3, 3)
    spec, eps = energy_spec(kind, dim), 2.0 * mc.ghmc_cases.step_size(kind, dim)
    g = torch.Generator().manual_seed(42)
    x0, v0 = torch.randn(n, dim, generator=g), torch.randn(n, dim, generator=g)
    z, u = torch.randn(n_mh, n, dim, generator=g), torch.rand(n_mh, n, generator=g)
    want = run_entry(dev, spec, x0, v0, n_mh, thin, L, eps, z=z, u=u)
    want_drawn = run_entry(dev, spec, x0, None, n_mh, thin, L, eps, seed=9, offset=5)
    for mass in (1.0, torch.ones(dim)):
        got = run_ghmc(dev, spec, mass, x0, v0, n_mh, thin, L, eps, z=z, u=u)
        drawn = run_ghmc(dev, spec, mass, x0, None, n_mh, thin, L, eps, seed=9, offset=5)
        for key in ("x", "v", "traj", "accepted"):
            assert torch.equal(got[key], want[key]) and torch.equal(drawn[key], want_drawn[key]), key
    assert want["accepted"].any() and (~want["accepted"]).any()


@gpu
@pytest.mark.parametrize("dim", [5, 100])
def test_the_transition_is_the_hmc_kernels_with_the_same_mass(cuda_device, dim):
    """gamma = inf, T = 1: c1 = 0, c2 = beta = 1 -- the chains are ebm_hmc_chain_f32 chains with the same diagonal mass, x and the
    mask bit for bit (double well at dims where that entry runs the lane-group kernel of the same geometry)."""
    dev, (n, n_mh, L) = cuda_device, (111, 5, 4)
    spec, mass = energy_spec("double_well", dim), mc.diag_mass(dim)
    eps = 0.15 * math.sqrt(mc.min_mass(mass))
    g = torch.Generator().manual_seed(21)
    x0, p0 = torch.randn(n, dim, generator=g), torch.randn(n, dim, generator=g)
    z, u = torch.randn(n_mh, n, dim, generator=g), torch.rand(n_mh, n, generator=g)
    got = run_ghmc(dev, spec, mass, x0, p0, n_mh, 1, L, eps, gamma=math.inf, temp=1.0, z=z, u=u)
    rows, p_d, u_d, m_d = x0.to(dev).clone(), z.to(dev), u.to(dev), mass.to(dev)
    mask = torch.empty(n_mh, n, dtype=torch.uint8, device=dev)
    _lib.call("ebm_hmc_chain_f32", model_of(spec, dev).fused_spec().to_c(), rows.data_ptr(), n, dim, n_mh, L, eps, None, _lib.MASS_DIAG,
              0.0, m_d.data_ptr(), 1, None, None, mask.data_ptr(), None, p_d.data_ptr(), u_d.data_ptr(), 0, 0, _lib.stream_handle(dev))
    torch.cuda.synchronize()
    assert torch.equal(mask.cpu().bool(), got["accepted"])
    assert (~got["accepted"]).any() and got["accepted"].any()
    assert torch.equal(rows.cpu(), got["x"])


# ---------------------------------------------------------------------------------
# draws and run structure
# ---------------------------------------------------------------------------------
def _field(dev, kind, seed, step, n_elem):
    out = torch.empty((n_elem + 3) // 4 * 4, device=dev)
    _lib.call("ebm_noise_fill_f32", out.data_ptr(), n_elem, kind, seed, step, _lib.stream_handle(dev))
    return out[:n_elem].clone()


def _start_momentum(dev, mass, sqrt_temp, seed, offset, n, dim):
    """(sqrt_temp m_sqrt) z0, z0 the normal field at step `offset`."""
    z0 = _field(dev, _lib.NOISE_NORMAL, seed, offset, n * dim).view(n, dim).cpu()
    return (sqrt_temp * mc.forms(mass, torch.float32)[1]) * z0


@gpu
@pytest.mark.parametrize("kind,dim,n,form", [("double_well", 5, 37, "diag"), ("harmonic", 100, 37, "scalar"), ("gmm", 32, 70, "diag"),
                                             ("gaussian", 256, 9, "scalar")])
def test_baoab_native_draws_are_the_materialised_fields(cuda_device, kind, dim, n, form):
    dev, (k, thin) = cuda_device, (11, 3)
    spec, mass = energy_spec(kind, dim), mc.mass_of(form, dim)
    h = mc.baoab_step(kind, mass)
    x0 = torch.randn(n, dim, generator=torch.Generator().manual_seed(5))
    seed, offset = 0x1234567887654321, 77
    p0 = _start_momentum(dev, mass, mc.kinetic_cases.constants(h, GAMMA, TEMP)[3], seed, offset, n, dim)
    noise = torch.stack([_field(dev, _lib.NOISE_NORMAL, seed, offset + 1 + s, n * dim) for s in range(k)]).view(k, n, dim).cpu()
    native = run_baoab(dev, spec, mass, x0, None, k, thin, h, seed=seed, offset=offset)
    fed = run_baoab(dev, spec, mass, x0, p0, k, thin, h, noise=noise)
    for key in ("x", "v", "traj"):
        assert torch.equal(native[key], fed[key]), key
        assert torch.isfinite(native[key]).all()
    mixed = run_baoab(dev, spec, mass, x0, None, k, thin, h, noise=noise, seed=seed, offset=offset)
    assert torch.equal(mixed["x"], fed["x"]) and torch.equal(mixed["v"], fed["v"])
    lo, hi = n // 3, n // 3 + max(n // 2, 1)  # a sub-block of chains run alone reproduces its rows of the full launch
    part = run_baoab(dev, spec, mass, x0[lo:hi], p0[lo:hi], k, thin, h, noise=noise[:, lo:hi])
    for key in ("x", "v", "traj"):
        assert torch.equal(part[key], fed[key][lo:hi]), key


@gpu
def test_ghmc_native_draws_are_the_materialised_fields(cuda_device):
    dev, (n_mh, thin) = cuda_device, (7, 3)
    rejected = 0
    for kind, dim, n, form in [("double_well", 5, 37, "diag"), ("harmonic", 100, 37, "scalar"), ("gmm", 32, 70, "diag"),
                               ("gaussian", 256, 9, "scalar")]:
        spec, mass, L = energy_spec(kind, dim), mc.mass_of(form, dim), mc.ghmc_cases.leapfrog_steps(dim)
        eps = 2.0 * mc.ghmc_step(kind, dim, mass)
        x0 = torch.randn(n, dim, generator=torch.Generator().manual_seed(5))
        seed, offset = 0x1234567887654321, 77
        p0 = _start_momentum(dev, mass, mc.ghmc_cases.constants(eps, L, GAMMA, TEMP)[2], seed, offset, n, dim)
        z = torch.stack([_field(dev, _lib.NOISE_NORMAL, seed, offset + 1 + 2 * t, n * dim) for t in range(n_mh)]).view(n_mh, n, dim).cpu()
        u = torch.stack([_field(dev, _lib.NOISE_UNIFORM, seed, offset + 2 + 2 * t, n) for t in range(n_mh)]).view(n_mh, n).cpu()
        native = run_ghmc(dev, spec, mass, x0, None, n_mh, thin, L, eps, seed=seed, offset=offset)
        fed = run_ghmc(dev, spec, mass, x0, p0, n_mh, thin, L, eps, z=z, u=u)
        for key in ("x", "v", "traj", "accepted"):
            assert torch.equal(native[key], fed[key]), (kind, key)
            assert torch.isfinite(native[key].float()).all()
        rejected += int((~native["accepted"]).sum())
        for kw in (dict(z=z), dict(u=u), dict(z=z, u=u)):
            mixed = run_ghmc(dev, spec, mass, x0, None, n_mh, thin, L, eps, seed=seed, offset=offset, **kw)
            assert torch.equal(mixed["x"], fed["x"]) and torch.equal(mixed["v"], fed["v"]), (kind, sorted(kw))
        lo, hi = n // 3, n // 3 + max(n // 2, 1)
        part = run_ghmc(dev, spec, mass, x0[lo:hi], p0[lo:hi], n_mh, thin, L, eps, z=z[:, lo:hi], u=u[:, lo:hi])
        for key in ("x", "v", "traj"):
            assert torch.equal(part[key], fed[key][lo:hi]), (kind, key)
        assert torch.equal(part["accepted"], fed["accepted"][:, lo:hi])
    assert rejected > 0, "no proposal was rejected: the accept uniforms were not exercised"


@gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind,dim", [("double_well", 5), ("gaussian", 100)])
def test_two_baoab_calls_are_one(cuda_device, kind, dim, form):
    dev, (n, k1, k2) = cuda_device, (37, 4, 7)
    spec, mass = energy_spec(kind, dim), mc.mass_of(form, dim)
    h = mc.baoab_step(kind, mass)
    x0 = torch.randn(n, dim, generator=torch.Generator().manual_seed(6))
    seed, offset = 0x0123456789ABCDEF, 41
    whole = run_baoab(dev, spec, mass, x0, None, k1 + k2, 1, h, seed=seed, offset=offset)
    first = run_baoab(dev, spec, mass, x0, None, k1, 1, h, seed=seed, offset=offset)
    second = run_baoab(dev, spec, mass, first["x"], first["v"], k2, 1, h, seed=seed, offset=offset + k1)
    assert torch.equal(second["x"], whole["x"]) and torch.equal(second["v"], whole["v"])
    assert torch.equal(torch.cat((first["traj"], second["traj"]), dim=1), whole["traj"])


@gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind,dim", [("double_well", 5), ("gmm", 100)])
def test_two_ghmc_calls_are_one(cuda_device, kind, dim, form):
    dev, (n, n1, n2) = cuda_device, (37, 4, 7)
    spec, mass, L = energy_spec(kind, dim), mc.mass_of(form, dim), mc.ghmc_cases.leapfrog_steps(dim)
    eps = 2.0 * mc.ghmc_step(kind, dim, mass)
    x0 = torch.randn(n, dim, generator=torch.Generator().manual_seed(6))
    seed, offset = 0x0123456789ABCDEF, 41
    whole = run_ghmc(dev, spec, mass, x0, None, n1 + n2, 1, L, eps, seed=seed, offset=offset)
    first = run_ghmc(dev, spec, mass, x0, None, n1, 1, L, eps, seed=seed, offset=offset)
    second = run_ghmc(dev, spec, mass, first["x"], first["v"], n2, 1, L, eps, seed=seed, offset=offset + 2 * n1)
    assert torch.equal(second["x"], whole["x"]) and torch.equal(second["v"], whole["v"])
    assert torch.equal(torch.cat((first["traj"], second["traj"]), dim=1), whole["traj"])
    assert torch.equal(torch.cat((first["accepted"], second["accepted"])), whole["accepted"])


# ---------------------------------------------------------------------------------
# buffers and stray values
# ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case", [mc.BAOAB_EXACT[1], mc.BAOAB_EXACT[9], mc.BAOAB_COUPLED[2], mc.BAOAB_COUPLED[7]])
def test_every_baoab_row_is_written_and_nothing_else(cuda_device, case):
    c = mc.baoab_case(*case)
    got = _run_baoab_case(cuda_device, c)  # (run_baoab checks the guards behind x, p, traj and the mass)
    lean = _run_baoab_case(cuda_device, c, traj=False)
    assert lean["traj"] is None and torch.equal(lean["x"], got["x"]) and torch.equal(lean["v"], got["v"])
    for key in ("x", "v", "traj"):
        assert not bool((got[key] == FILL).any()), f"a slot of {key} was not written"
    drawn = run_baoab(cuda_device, c["spec"], c["mass"], c["x0"], None, c["k"], c["thin"], c["h"], noise=c["noise"], seed=3, offset=9)
    assert not bool((drawn["v"] == FILL).any()) and torch.isfinite(drawn["v"]).all()


@gpu
@pytest.mark.parametrize("case", [mc.GHMC_CASES[1], mc.GHMC_CASES[8], mc.GHMC_CASES[9], mc.GHMC_CASES[16]])
def test_every_ghmc_row_is_written_and_nothing_else(cuda_device, case):
    c = mc.ghmc_case(*case)
    got = _run_ghmc_case(cuda_device, c)
    lean = _run_ghmc_case(cuda_device, c, traj=False, mask=False)
    assert lean["traj"] is None and lean["accepted"] is None and torch.equal(lean["x"], got["x"]) and torch.equal(lean["v"], got["v"])
    for key in ("x", "v", "traj"):
        assert not bool((got[key] == FILL).any()), f"a slot of {key} was not written"
    drawn = run_ghmc(cuda_device, c["spec"], c["mass"], c["x0"], None, c["n_mh"], c["thin"], c["L"], c["eps"], z=c["z"], u=c["u"], seed=3,
                     offset=9)
    assert not bool((drawn["v"] == FILL).any()) and torch.isfinite(drawn["v"]).all()


def _wild(x0):
    x0 = x0.clone()
    x0[3, 2] = float("nan")
    x0[7, 4] = 1e20
    return x0, [i for i in range(x0.shape[0]) if i not in (3, 7)]


@gpu
@pytest.mark.parametrize("case", [mc.BAOAB_EXACT[1], mc.BAOAB_COUPLED[0]])
def test_a_wild_baoab_start_stays_in_its_chain(cuda_device, case):
    c = mc.baoab_case(*case)
    x0, others = _wild(c["x0"])
    got = run_baoab(cuda_device, c["spec"], c["mass"], x0, c["v0"], c["k"], c["thin"], c["h"], noise=c["noise"])
    clean = _run_baoab_case(cuda_device, c)
    for key in ("x", "v", "traj"):
        assert torch.isfinite(clean[key]).all() and torch.equal(got[key][others], clean[key][others]), key
    assert torch.isnan(got["x"][3]).any()


@gpu
@pytest.mark.parametrize("case", [mc.GHMC_CASES[1], mc.GHMC_CASES[9]])
def test_a_wild_ghmc_start_stays_in_its_chain(cuda_device, case):
    c = mc.ghmc_case(*case)
    x0, others = _wild(c["x0"])
    got = run_ghmc(cuda_device, c["spec"], c["mass"], x0, c["v0"], c["n_mh"], c["thin"], c["L"], c["eps"], z=c["z"], u=c["u"])
    clean = _run_ghmc_case(cuda_device, c)
    for key in ("x", "v", "traj"):
        assert torch.isfinite(clean[key]).all() and torch.equal(got[key][others], clean[key][others]), key
    assert torch.equal(got["accepted"][:, others], clean["accepted"][:, others])
    assert torch.isnan(got["x"][3]).any() and not got["accepted"][:, 3].any()  # the NaN chain held its state and only flipped


@gpu
def test_refusals_launch_nothing(cuda_device):
    """The refusals of test_mass.py with real buffers: each raises its code and no buffer, the mass included, is touched."""
    from test_mass import baoab_abi_call, baoab_refusals, ghmc_abi_call, ghmc_refusals

    dev, (n, dim) = cuda_device, (4, 8)
    x = torch.full((n, 260), FILL, device=dev)
    v = torch.full((n, 260), FILL, device=dev)
    m = torch.full((260,), FILL, device=dev)
    real = dict(x=x.data_ptr(), v=v.data_ptr())
    desc = model_of(energy_spec("double_well", dim), dev).fused_spec().to_c()
    mlp = ta.MLPEnergy(dim, 64, device=dev)
    for call, refusals in ((baoab_abi_call, baoab_refusals), (ghmc_abi_call, ghmc_refusals)):
        for kw, exc, match in refusals():
            with pytest.raises(exc, match=match):
                call(desc, **{**real, **kw})
        for kw, exc, match in refusals()[:5]:  # ... and what the unit-mass entry refuses, with a diagonal mass at hand
            with pytest.raises(exc, match=match):
                call(desc, **{**real, "mass_kind": _lib.MASS_DIAG, "diag": m.data_ptr(), **kw})
        with pytest.raises(RuntimeError, match=r"code -2"):
            call(mlp.fused_spec().to_c(), **real)
    torch.cuda.synchronize()
    for t in (x, v, m):
        assert bool((t == FILL).all())


# ---------------------------------------------------------------------------------
# through sample()
# ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("form", FORMS)
def test_baoab_sample_is_one_launch(cuda_device, form):
    dev, (n, dim, k1, k2) = cuda_device, (300, 6, 17, 23)
    k = k1 + k2
    spec, mass = energy_spec("double_well", dim), mc.mass_of(form, dim)
    h = mc.baoab_step("double_well", mass)
    x0 = torch.randn(n, dim, device=dev)
    keep = x0.clone()
    s = ta.UnderdampedLangevin(model_of(spec, dev), step_size=h, friction=GAMMA, temperature=TEMP, device=dev, mass=mass)
    assert s._route(x0)[0] == "fused_mass" and (form == "scalar" or s.mass.is_cuda)
    keep_mass = None if form == "scalar" else s.mass.clone()
    g = torch.Generator(device=dev).manual_seed(5)
    before = dict(_lib.call_counts)
    x, p = s.sample(x=x0, n_steps=k, return_velocity=True, generator=g)
    torch.cuda.synchronize()
    new = {name: c - before.get(name, 0) for name, c in _lib.call_counts.items() if c != before.get(name, 0)}
    assert new == {BAOAB_ENTRY: 1}, new
    assert _rng._get_offset(g) == 4 * (k + 1)
    assert torch.equal(x0, keep) and (form == "scalar" or torch.equal(s.mass, keep_mass)), "the caller's tensors were touched"
    want = run_baoab(dev, spec, mass, x0.cpu(), None, k, 1, h, seed=_rng.kernel_seed(5), offset=0)
    assert torch.equal(x.cpu(), want["x"]) and torch.equal(p.cpu(), want["v"]) and torch.isfinite(x).all()
    # cut in two: the second call continues from the returned momentum at the Philox step the first one stopped at
    g = torch.Generator(device=dev).manual_seed(5)
    xa, pa = s.sample(x=x0, n_steps=k1, return_velocity=True, generator=g)
    _rng._set_offset(g, 4 * k1)
    pa_keep = pa.clone()
    xb, pb = s.sample(x=xa, n_steps=k2, velocity=pa, return_velocity=True, reset_schedulers=False, generator=g)
    assert torch.equal(pa, pa_keep) and torch.equal(xb, x) and torch.equal(pb, p)
    traj, diag = s.sample(x=x0, n_steps=k, thin=4, return_trajectory=True, return_diagnostics=True,
                          generator=torch.Generator(device=dev).manual_seed(5))
    assert traj.shape == (n, k // 4, dim) and torch.equal(traj[:, -1], x)
    m = mass if form == "scalar" else mass.to(dev)
    assert torch.allclose(diag["kinetic_temperature"], (p.square() / m).mean())  # the mean of p^2 / m


@gpu
@pytest.mark.parametrize("form", FORMS)
def test_ghmc_sample_is_one_launch(cuda_device, form):
    dev, (n, dim, k1, k2, L) = cuda_device, (300, 6, 17, 23, 3)
    k = k1 + k2
    spec, mass = energy_spec("double_well", dim), mc.mass_of(form, dim)
    eps = 0.2 * math.sqrt(mc.min_mass(mass))
    x0 = torch.randn(n, dim, device=dev)
    keep = x0.clone()
    s = ta.GeneralizedHMC(model_of(spec, dev), step_size=eps, n_leapfrog_steps=L, friction=GAMMA, temperature=TEMP, device=dev, mass=mass)
    assert s._route(x0)[0] == "fused_mass"
    keep_mass = None if form == "scalar" else s.mass.clone()
    g = torch.Generator(device=dev).manual_seed(5)
    before = dict(_lib.call_counts)
    x, p = s.sample(x=x0, n_steps=k, return_velocity=True, generator=g)
    torch.cuda.synchronize()
    new = {name: c - before.get(name, 0) for name, c in _lib.call_counts.items() if c != before.get(name, 0)}
    assert new == {GHMC_ENTRY: 1}, new
    assert _rng._get_offset(g) == 4 * (2 * k + 1)
    assert torch.equal(x0, keep) and (form == "scalar" or torch.equal(s.mass, keep_mass)), "the caller's tensors were touched"
    want = run_ghmc(dev, spec, mass, x0.cpu(), None, k, 1, L, eps, seed=_rng.kernel_seed(5), offset=0)
    assert torch.equal(x.cpu(), want["x"]) and torch.equal(p.cpu(), want["v"])
    assert want["accepted"].any() and (~want["accepted"]).any()
    g = torch.Generator(device=dev).manual_seed(5)
    xa, pa = s.sample(x=x0, n_steps=k1, return_velocity=True, generator=g)
    _rng._set_offset(g, 4 * 2 * k1)
    xb, pb = s.sample(x=xa, n_steps=k2, velocity=pa, return_velocity=True, reset_schedulers=False, generator=g)
    assert torch.equal(xb, x) and torch.equal(pb, p)
    traj, diag = s.sample(x=x0, n_steps=k, thin=4, return_trajectory=True, return_diagnostics=True,
                          generator=torch.Generator(device=dev).manual_seed(5))
    assert traj.shape == (n, k // 4, dim) and torch.equal(traj[:, -1], x)
    assert torch.allclose(diag["acceptance_rate"].cpu(), want["accepted"][3::4][: k // 4].float().mean(dim=1), rtol=0, atol=1e-6)
    m = mass if form == "scalar" else mass.to(dev)
    assert torch.allclose(diag["kinetic_temperature"], (p.square() / m).mean())


@gpu
@pytest.mark.parametrize("cls,entry", [(ta.UnderdampedLangevin, BAOAB_ENTRY), (ta.GeneralizedHMC, GHMC_ENTRY)])
def test_other_configurations_take_the_eager_route_on_the_gpu(cuda_device, cls, entry):
    """A scheduler on the step size, a row wider than 256 and an MLPEnergy (opted in or not): the torch-op recurrence, no launch of the
    massed entry; the states stay finite and on the device."""
    dev, n = cuda_device, 64
    before = hip_calls(entry)
    configs = [(4, ta.HarmonicModel(k=4.0, device=dev), ta.core.schedules.LinearScheduler(0.3, 0.1, 10), False),
               (300, ta.HarmonicModel(k=4.0, device=dev), 0.1, False),
               (8, ta.MLPEnergy(8, 64, device=dev), 0.01, False),
               (8, ta.MLPEnergy(8, 64, device=dev), 0.01, True)]
    for dim, model, step, opt_in in configs:
        for mass in (0.37, mc.diag_mass(dim)):
            s = cls(model, step_size=step, device=dev, mass=mass)
            s.fused_mlp = opt_in
            x0 = 0.5 * torch.randn(n, dim, device=dev)
            assert s._route(x0)[0] == "eager"
            x, p = s.sample(x=x0, n_steps=4, return_velocity=True)
            assert x.is_cuda and p.is_cuda and x.shape == p.shape == (n, dim) and torch.isfinite(x).all() and torch.isfinite(p).all()
    assert hip_calls(entry) == before


@gpu
def test_sample_moments_of_a_massed_sampler_stays_step_by_step(cuda_device):
    dev = cuda_device
    mass = torch.tensor(mc.LAW_MASS)
    s = ta.UnderdampedLangevin(mc.law_model(dev), step_size=mc.LAW_STEP, friction=mc.LAW_GAMMA_BAOAB, temperature=mc.LAW_TEMP, device=dev,
                               mass=mass)
    before = dict(_lib.call_counts)
    x0 = mc.law_start(dev)[:1024]
    _, mom, p = s.sample_moments(x=x0, n_steps=6, return_velocity=True, generator=torch.Generator(device=dev).manual_seed(1))
    assert _lib.call_counts["ebm_kinetic_moments_f32"] == before.get("ebm_kinetic_moments_f32", 0)
    assert _lib.call_counts[BAOAB_ENTRY] == before.get(BAOAB_ENTRY, 0) + 6
    # the same six launches by hand: the v^2 average is that of p^2 / m
    g, x, q, seen = torch.Generator(device=dev).manual_seed(1), x0, None, []
    for _ in range(6):
        x, q = s.sample(x=x, n_steps=1, velocity=q, return_velocity=True, reset_schedulers=False, generator=g)
        seen.append(q * q / s.mass)
    assert torch.equal(q, p)
    assert torch.allclose(mom.kinetic_temperature, torch.stack(seen).double().mean(dim=(0, 1)), rtol=1e-5)


# ---------------------------------------------------------------------------------
# the laws on the fused route
# ---------------------------------------------------------------------------------
@gpu
def test_the_baoab_law_holds_on_the_fused_route(cuda_device):
    dev = cuda_device
    s = ta.UnderdampedLangevin(mc.law_model(dev), step_size=mc.LAW_STEP, friction=mc.LAW_GAMMA_BAOAB, temperature=mc.LAW_TEMP, device=dev,
                               mass=torch.tensor(mc.LAW_MASS))
    before = hip_calls(BAOAB_ENTRY)
    x, p = s.sample(x=mc.law_start(dev), n_steps=mc.LAW_STEPS, return_velocity=True, generator=torch.Generator(device=dev).manual_seed(mc.LAW_SEED))
    assert hip_calls(BAOAB_ENTRY) == before + 1
    mc.check_law(x.cpu(), p.cpu(), baoab=True)


@gpu
def test_the_ghmc_law_holds_on_the_fused_route(cuda_device):
    dev = cuda_device
    s = ta.GeneralizedHMC(mc.law_model(dev), step_size=mc.LAW_STEP, n_leapfrog_steps=1, friction=mc.LAW_GAMMA_GHMC, temperature=mc.LAW_TEMP,
                          device=dev, mass=torch.tensor(mc.LAW_MASS))
    before = hip_calls(GHMC_ENTRY)
    x, diag, p = s.sample(x=mc.law_start(dev), n_steps=mc.LAW_STEPS, thin=mc.LAW_STEPS // 4, return_diagnostics=True, return_velocity=True,
                          generator=torch.Generator(device=dev).manual_seed(mc.LAW_SEED))
    assert hip_calls(GHMC_ENTRY) == before + 1
    mc.check_law(x.cpu(), p.cpu(), baoab=False)
    assert 0.5 < diag["acceptance_rate"].mean().item() < 1.0
