"""ebm_kinetic_mlp_chain_mass_f32, ebm_ghmc_mlp_chain_mass_f32 and the ``fused_mlp_mass`` opt-in of UnderdampedLangevin and
GeneralizedHMC without a GPU: the exports and their declarations, the refusals the entries make in front of any device access,
the opt-in's default and CPU behaviour, the conditions every GPU case must meet (docs/design/mass_mlp.md), and the one launch
of the opted-in route against a recording stand-in of the library."""

import os
import re

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib, _rng
from helpers import fused_cpu  # noqa: F401  (the fixture)
import mass_mlp_cases as mm

BAOAB_ENTRY, GHMC_ENTRY = "ebm_kinetic_mlp_chain_mass_f32", "ebm_ghmc_mlp_chain_mass_f32"
INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
HEADER, COMPANION = os.path.join(INCLUDE, "ebm_hip.h"), os.path.join(INCLUDE, "ebm_hip_mass_mlp.h")
FORMS = ("scalar", "diag")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def test_the_entries_are_exported_and_declared():
    """Fails without the feature."""
    with open(HEADER) as fh:  # the companion header declares the two; the unit-mass lists they extend are ebm_hip.h's
        header = fh.read()
    with open(COMPANION) as fh:
        companion = fh.read()
    assert '#include "ebm_hip.h"' in companion and sorted(re.findall(r"EBM_API\s+int\s+(ebm_\w+)\s*\(", companion)) == sorted(
        _lib.EXPORTS_MASS_MLP) == sorted((BAOAB_ENTRY, GHMC_ENTRY))
    header = header + companion

    def params(name):
        m = re.search(r"EBM_API\s+int\s+" + name + r"\s*\(([^)]*)\)", header)
        assert m, name
        return re.sub(r"\s+", " ", m.group(1)).strip()

    three = "int32_t mass_kind, double mass_scalar, const float* mass_diag, "
    for entry, unit, behind in ((BAOAB_ENTRY, "ebm_kinetic_mlp_chain_f32", 7), (GHMC_ENTRY, "ebm_ghmc_mlp_chain_f32", 9)):
        assert entry in _lib.EXPORTS_MASS_MLP and entry in _lib._PROTOTYPES and hasattr(_lib.lib(), entry)
        assert params(entry) == params(unit).replace("double temperature, ", "double temperature, " + three)
        proto, unit_proto = _lib._PROTOTYPES[entry][1], _lib._PROTOTYPES[unit][1]
        at = len(unit_proto) - behind  # behind `temperature`
        assert proto == unit_proto[:at] + [_lib._i32, _lib._d, _lib._p] + unit_proto[at:]
    # the analytic massed entries take the same lists
    assert _lib._PROTOTYPES[BAOAB_ENTRY] == _lib._PROTOTYPES["ebm_kinetic_chain_mass_f32"]
    assert _lib._PROTOTYPES[GHMC_ENTRY] == _lib._PROTOTYPES["ebm_ghmc_chain_mass_f32"]
    assert _lib.ABI_VERSION == 9 and _lib.lib().ebm_version() == 9


# ---------------------------------------------------------------------------------
# the refusals of the two entries
# ---------------------------------------------------------------------------------
def _mlp_desc(hidden):
    desc = _lib.EnergyDesc()
    desc.kind, desc.n_comp, desc.dev0 = _lib.ENERGY_MLP, hidden, 16
    return desc


def baoab_abi_call(desc, *, x=16, v=16, n=4, dim=8, k=3, h=0.1, gamma=1.0, temp=1.0, mass_kind=_lib.MASS_SCALAR, mass=0.5, diag=None,
                   thin=1):
    _lib.call(BAOAB_ENTRY, desc, x, v, n, dim, k, h, gamma, temp, mass_kind, mass, diag, 0, thin, None, None, 0, 0, None)


def ghmc_abi_call(desc, *, x=16, v=16, n=4, dim=8, n_mh=3, L=2, eps=0.1, gamma=1.0, temp=1.0, mass_kind=_lib.MASS_SCALAR, mass=0.5,
                  diag=None, thin=1):
    _lib.call(GHMC_ENTRY, desc, x, v, n, dim, n_mh, L, eps, gamma, temp, mass_kind, mass, diag, 0, thin, None, None, None, None, 0, 0, None)


MASS_REFUSALS = [
    (dict(mass_kind=_lib.MASS_NONE), "mass_kind=0"),
    (dict(mass_kind=3), "mass_kind=3"),
    (dict(mass_kind=-1), "mass_kind=-1"),
    (dict(mass_kind=_lib.MASS_DIAG, diag=None), "mass_diag is NULL"),
    (dict(mass=0.0), "mass_scalar=0 "),
    (dict(mass=-2.0), "mass_scalar=-2"),
    (dict(mass=float("inf")), "mass_scalar=inf"),
    (dict(mass=float("nan")), "mass_scalar=nan"),
]


def _unit_refusals(baoab):
    if baoab:
        from test_kinetic_mlp import EINVAL
    else:
        from test_ghmc_mlp import EINVAL
    return EINVAL


@pytest.mark.parametrize("baoab", [True, False], ids=["baoab", "ghmc"])
def test_abi_refusals_need_no_gpu(baoab):
    """The unit-mass MLP entry's refusals and those of the mass, in front of any device access (the pointers are never
    dereferenced) and of the early return of an empty call; a mass refusal comes behind the walk's own checks and the shape rule."""
    call = baoab_abi_call if baoab else ghmc_abi_call
    desc = _mlp_desc(64)
    for n in (4, 0):
        with pytest.raises(ValueError, match="energy descriptor is NULL"):
            call(None, n=n)
        for kw, match in _unit_refusals(baoab) + MASS_REFUSALS:  # EBM_EINVAL
            with pytest.raises(ValueError, match=match):
                call(desc, n=n, **kw)
        for kind in (_lib.ENERGY_DOUBLE_WELL, _lib.ENERGY_HARMONIC, _lib.ENERGY_ROSENBROCK, _lib.ENERGY_ACKLEY,
                     _lib.ENERGY_RASTRIGIN):
            other = _lib.EnergyDesc()
            other.kind = kind
            with pytest.raises(RuntimeError, match=r"code -2.*MLP energy only.*chain_mass_f32 takes the analytic kinds"):  # EBM_EKIND
                call(other, n=n)
        with pytest.raises(RuntimeError, match=r"code -3.*hidden width 64 or 128.*got 96, 8"):  # EBM_EDIM
            call(_mlp_desc(96), n=n)
        with pytest.raises(RuntimeError, match=r"code -3.*hidden width 64 or 128.*got 256, 8"):
            call(_mlp_desc(256), n=n)
        with pytest.raises(RuntimeError, match=r"code -3.*1 <= dim <= 128.*got 64, 129"):
            call(desc, n=n, dim=129)
        with pytest.raises(RuntimeError, match=r"code -3.*got 128, 0"):
            call(_mlp_desc(128), n=n, dim=0)
        # the order: the walk's parameters and the shape rule in front of the mass
        with pytest.raises(ValueError, match="thin=0"):
            call(desc, n=n, thin=0, mass_kind=_lib.MASS_NONE)
        with pytest.raises(RuntimeError, match=r"code -3.*got 64, 129"):
            call(desc, n=n, dim=129, mass=-1.0)
    call(desc, n=0)  # an empty call returns in front of any launch
    call(_mlp_desc(128), n=0, dim=128, mass_kind=_lib.MASS_DIAG, diag=16)
    # the unit-mass MLP entries and the analytic massed entries are untouched
    with pytest.raises(RuntimeError, match=r"code -2.*no (underdamped-Langevin|generalized-HMC) kernel"):
        _lib.call("ebm_kinetic_chain_mass_f32" if baoab else "ebm_ghmc_chain_mass_f32", desc, 16, 16, 4, 8, 3, *((0.1,) if baoab else (2, 0.1)),
                  1.0, 1.0, _lib.MASS_SCALAR, 0.5, None, 0, 1, None, *((None,) if baoab else (None, None, None)), 0, 0, None)


# ---------------------------------------------------------------------------------
# the opt-in
# ---------------------------------------------------------------------------------
class AsCuda:  # what _route reads of a state, with no GPU at hand
    def __init__(self, dim, dtype=torch.float32, ndim=2):
        self.is_cuda, self.dtype, self.ndim, self.shape, self.device = True, dtype, ndim, (8, dim), torch.device("cpu")


@pytest.fixture
def mlp_spec_on_cpu(monkeypatch):
    """An MLPEnergy on the CPU has no fused spec.  The samplers' `fused_spec_for` hands out one over its packed parameters here
    (what the model builds on a GPU), so that `_route` itself -- the opt-ins, the mass, the shape rule -- runs without one."""
    import torchebm_amd.samplers.ghmc as ghmc_mod
    import torchebm_amd.samplers.kinetic as kinetic_mod

    real = kinetic_mod.fused_spec_for

    def spec_for(model, x, model_kwargs, **kw):
        if isinstance(model, ta.MLPEnergy) and not model_kwargs and x.ndim == 2:
            return ta.core.energies.FusedSpec(_lib.ENERGY_MLP, n_comp=model.hidden, dev0=model._packed_parameters(), langevin_only=True,
                                              dim=model.in_dim, hmc=True)
        return real(model, x, model_kwargs, **kw)

    monkeypatch.setattr(kinetic_mod, "fused_spec_for", spec_for)
    monkeypatch.setattr(ghmc_mod, "fused_spec_for", spec_for)


@pytest.mark.parametrize("cls,extra", [(ta.UnderdampedLangevin, {}), (ta.GeneralizedHMC, dict(n_leapfrog_steps=3))], ids=["baoab", "ghmc"])
def test_the_opt_in_is_off_by_default_and_changes_nothing_on_the_cpu(cls, extra):
    assert cls.fused_mlp_mass is False
    torch.manual_seed(4)
    model = ta.MLPEnergy(4, 64)
    for mass in (0.37, mm.mass_of("diag", 4)):
        kw = dict(step_size=0.2, friction=1.5, temperature=0.8, mass=mass, **extra)
        plain, opted = cls(model, **kw), cls(model, **kw)
        assert plain.fused_mlp_mass is False
        opted.fused_mlp = opted.fused_mlp_mass = True
        x0 = torch.randn(48, 4, generator=_gen(1))
        assert plain._route(x0)[0] == "eager" and opted._route(x0)[0] == "eager" and opted._route(x0, {})[0] == "eager"  # CPU states
        a = plain.sample(x=x0, n_steps=7, thin=2, return_trajectory=True, return_diagnostics=True, return_velocity=True, generator=_gen(9))
        b = opted.sample(x=x0, n_steps=7, thin=2, return_trajectory=True, return_diagnostics=True, return_velocity=True, generator=_gen(9))
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and a[0].shape == (48, 3, 4)
        for key in ("mean", "var", "energy", "kinetic_temperature"):
            assert torch.equal(a[1][key], b[1][key]), key
        assert torch.isfinite(a[0]).all() and torch.isfinite(a[2]).all()


@pytest.mark.parametrize("cls", [ta.UnderdampedLangevin, ta.GeneralizedHMC])
def test_routing_needs_both_opt_ins_and_the_conditions_of_fused_mlp(cls, mlp_spec_on_cpu):
    """Fails without the feature."""
    for mass in (0.37, torch.ones(8)):
        s = cls(ta.MLPEnergy(8, 64), step_size=0.01, mass=mass)
        assert s._route(AsCuda(8))[0] == "eager"
        s.fused_mlp = True  # fused_mlp alone leaves a massed MLP sampler eager
        assert s._route(AsCuda(8))[0] == "eager"
        s.fused_mlp_mass = True
        route, spec = s._route(AsCuda(8))
        assert route == "fused_mlp_mass" and spec.kind == _lib.ENERGY_MLP and spec.n_comp == 64
        assert s._route(torch.zeros(3, 8)) == ("eager", None)  # a CPU state
        assert s._route(AsCuda(8), {"c": 1})[0] == "eager" and s._route(AsCuda(8, torch.float64))[0] == "eager"
        assert s._route(AsCuda(8, ndim=3))[0] == "eager" and s._route(AsCuda(7))[0] == "eager"  # dim != in_dim
        s.fused_mlp = False  # fused_mlp_mass alone is no opt-in
        assert s._route(AsCuda(8))[0] == "eager"
        wide = cls(ta.MLPEnergy(8, 96), step_size=0.01, mass=mass)  # off the shapes
        wide.fused_mlp = wide.fused_mlp_mass = True
        assert wide._route(AsCuda(8))[0] == "eager"
        sched = cls(ta.MLPEnergy(8, 64), step_size=ta.core.schedules.LinearScheduler(0.3, 0.1, 10), mass=mass)
        sched.fused_mlp = sched.fused_mlp_mass = True
        assert sched._route(AsCuda(8))[0] == "eager"
    both = cls(ta.MLPEnergy(8, 64), step_size=0.01)  # without a mass the second opt-in changes nothing
    both.fused_mlp = both.fused_mlp_mass = True
    assert both._route(AsCuda(8))[0] == "fused_mlp"
    analytic = cls(ta.DoubleWellModel(), step_size=0.05, mass=0.37)
    analytic.fused_mlp = analytic.fused_mlp_mass = True
    assert analytic._route(AsCuda(8))[0] == "fused_mass"


# ---------------------------------------------------------------------------------
# the GPU cases
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("in_dim,hidden,n,k,thin,form", mm.BAOAB_CASES)
def test_the_fp32_restatement_of_every_baoab_case_tracks_fp64(in_dim, hidden, n, k, thin, form):
    c = mm.baoab_case(in_dim, hidden, n, k, thin, form)
    assert c["ref64"]["traj"].shape == (n, k // thin, in_dim)
    for key, (err, scale) in mm.restatement_errors(c).items():
        print(f"BAOAB dim {in_dim} H {hidden} n {n} k {k} {form}: {key} fp32 err {err:.3e} max|ref| {scale:.3e}")
        assert err <= 1e-4 * scale, (key, err, scale)


@pytest.mark.parametrize("in_dim,hidden,n,n_mh,thin,L,form", mm.GHMC_CASES)
def test_every_ghmc_case_meets_its_conditions(in_dim, hidden, n, n_mh, thin, L, form):
    c = mm.ghmc_case(in_dim, hidden, n, n_mh, thin, L, form)
    acc = c["ref64"]["accepted"]
    print(f"GHMC dim {in_dim} H {hidden} n {n} n_mh {n_mh} L {L} {form}: seed {c['seed']} margin {c['ref64']['margin']:.3e} "
          f"accepted {int(acc.sum())} rejected {int((~acc).sum())}")
    assert c["found"] and c["seed"] < mm.MAX_SEEDS
    assert c["ref64"]["margin"] > mm.MARGIN_BAR and torch.equal(c["ref32"]["accepted"], acc)
    assert int(acc.sum()) >= mm.MIN_DECISIONS and int((~acc).sum()) >= mm.MIN_DECISIONS
    assert acc.shape == (n_mh, n) and c["ref64"]["traj"].shape == (n, n_mh // thin, in_dim)
    for key, (err, scale) in mm.restatement_errors(c).items():
        print(f"    {key} fp32 err {err:.3e} max|ref| {scale:.3e}")
        assert err <= 1e-4 * scale, (key, err, scale)


def test_the_cases_cover_every_kernel_and_both_forms():
    for cases, per in ((mm.BAOAB_CASES, 5), (mm.GHMC_CASES, 6)):
        assert len(cases) == 12
        assert {(c[1], (c[0] + 31) // 32) for c in cases} == {(h, dt) for h in (64, 128) for dt in (1, 2, 3, 4)}
        assert {c[per] for c in cases} == set(FORMS)
        assert any(c[0] % 4 for c in cases) and any(c[0] % 4 == 0 for c in cases)  # both Philox paths
        assert any(c[0] % 32 and c[per] == "diag" for c in cases)  # padded columns under a diagonal mass
        assert {c[2] for c in cases} == {37, 129, 257}
    assert {(c[1], (c[0] + 31) // 32) for c in mm.ANCHOR_SHAPES} == {(h, dt) for h in (64, 128) for dt in (1, 2, 3, 4)}
    assert [d for d, _ in mm.PHILOX_DIMS] == [5, 33, 40, 128]


# ---------------------------------------------------------------------------------
# the opted-in route against the recording stand-in
# ---------------------------------------------------------------------------------
def _opted(fused_cpu, cls, mass, route_of=None, **kw):  # noqa: F811
    """A sampler on an MLPEnergy(5, 64) with a CPU `spec`; `_route` is the sampler's own, run on a stand-in for a CUDA state."""
    make, rec, clones = fused_cpu
    torch.manual_seed(8)
    model = ta.MLPEnergy(5, 64)
    s = cls(model, step_size=0.2, friction=1.5, temperature=0.8, mass=mass, device="cpu", **kw)
    return s, rec, clones


def _route_as_cuda(monkeypatch, s):
    own = type(s)._route
    monkeypatch.setattr(s, "_route", lambda x, model_kwargs=None: own(s, AsCuda(x.shape[1]), model_kwargs))


@pytest.mark.parametrize("form", FORMS)
def test_the_opted_in_baoab_route_is_one_launch_of_the_entry(fused_cpu, monkeypatch, mlp_spec_on_cpu, form):  # noqa: F811
    """Fails without the feature."""
    mass = 0.37 if form == "scalar" else mm.mass_of("diag", 5)
    s, rec, _ = _opted(fused_cpu, ta.UnderdampedLangevin, mass)
    _route_as_cuda(monkeypatch, s)
    reserved = []
    monkeypatch.setattr(_rng, "reserve", lambda generator, device, n_steps: reserved.append(n_steps) or (7, 11))
    n, dim, k, thin = 37, 5, 11, 3
    x0, v0 = torch.randn(n, dim, generator=_gen(1)), torch.randn(n, dim, generator=_gen(2))
    keep = (x0.clone(), v0.clone())
    s.fused_mlp = True  # alone: eager, nothing recorded
    s.sample(x=x0, n_steps=k, generator=_gen(3))
    assert not rec.named("ebm_") and reserved == []
    s.fused_mlp_mass = True
    x, p = s.sample(x=x0, n_steps=k, thin=thin, return_velocity=True, generator=_gen(3))
    assert reserved == [k + 1] and [name for name, _ in rec.named("ebm_")] == [BAOAB_ENTRY]
    args = rec.calls[0][1]
    # (energy, x, v, n, dim, k, h, gamma, T, mass_kind, mass_scalar, mass_diag, draw_v0, thin, traj, noise, seed, offset, stream)
    assert args[1] == x.data_ptr() != x0.data_ptr() and args[2] == p.data_ptr() and tuple(args[3:9]) == (n, dim, k, 0.2, 1.5, 0.8)
    if form == "scalar":
        assert tuple(args[9:12]) == (_lib.MASS_SCALAR, 0.37, None)
    else:
        assert args[9] == _lib.MASS_DIAG and args[10] == 0.0 and args[11] == s.mass.data_ptr()
    assert tuple(args[12:]) == (1, thin, None, None, 7, 11, None)
    # a momentum given: read, cloned, never the caller's; a trajectory asked for: its buffer is passed
    rec.calls.clear()
    traj, p = s.sample(x=x0, n_steps=k, thin=thin, velocity=v0, return_trajectory=True, return_velocity=True, generator=_gen(3))
    (name, args), = rec.named("ebm_")
    assert name == BAOAB_ENTRY and args[12] == 0 and args[2] == p.data_ptr() != v0.data_ptr()
    assert args[14] == traj.data_ptr() and traj.shape == (n, k // thin, dim)
    assert torch.equal(x0, keep[0]) and torch.equal(v0, keep[1])
    # no step: no launch of the entry; the start momentum alone comes from the noise field
    rec.calls.clear()
    x, p = s.sample(x=torch.ones(8, 5), n_steps=0, return_velocity=True)
    assert [name for name, _ in rec.named("ebm_")] == ["ebm_noise_fill_f32"] and torch.equal(x, torch.ones(8, 5)) and p.shape == (8, 5)


@pytest.mark.parametrize("form", FORMS)
def test_the_opted_in_ghmc_route_is_one_launch_of_the_entry(fused_cpu, monkeypatch, mlp_spec_on_cpu, form):  # noqa: F811
    """Fails without the feature."""
    mass = 0.37 if form == "scalar" else mm.mass_of("diag", 5)
    s, rec, _ = _opted(fused_cpu, ta.GeneralizedHMC, mass, n_leapfrog_steps=3)
    _route_as_cuda(monkeypatch, s)
    reserved = []
    monkeypatch.setattr(_rng, "reserve", lambda generator, device, n_steps: reserved.append(n_steps) or (7, 11))
    n, dim, n_mh, thin = 37, 5, 5, 2
    x0, v0 = torch.randn(n, dim, generator=_gen(1)), torch.ones(n, dim)
    s.fused_mlp = True  # alone: eager, nothing recorded
    s.sample(x=x0, n_steps=n_mh, generator=_gen(3))
    assert not rec.named("ebm_") and reserved == []
    s.fused_mlp_mass = True
    traj, diag, p = s.sample(x=x0, n_steps=n_mh, thin=thin, velocity=v0, return_trajectory=True, return_diagnostics=True, return_velocity=True)
    assert reserved == [2 * n_mh + 1] and [name for name, _ in rec.named("ebm_")] == [GHMC_ENTRY]
    name, args = rec.calls[0]
    # (energy, x, v, n, dim, n_mh, L, eps, gamma, T, mass_kind, mass_scalar, mass_diag, draw_v0, thin, traj, mask, noise, u, seed, offset, stream)
    assert args[2] == p.data_ptr() != v0.data_ptr() and torch.equal(v0, torch.ones(n, dim))
    assert tuple(args[3:10]) == (n, dim, n_mh, 3, 0.2, 1.5, 0.8)
    if form == "scalar":
        assert tuple(args[10:13]) == (_lib.MASS_SCALAR, 0.37, None)
    else:
        assert args[10] == _lib.MASS_DIAG and args[11] == 0.0 and args[12] == s.mass.data_ptr()
    assert tuple(args[13:16]) == (0, thin, traj.data_ptr()) and args[16] is not None and tuple(args[17:]) == (None, None, 7, 11, None)
    assert "kinetic_temperature" in diag and diag["acceptance_rate"].shape == (n_mh // thin,)
    rec.calls.clear()
    s.sample(x=x0, n_steps=n_mh)  # the start momentum drawn in the launch
    (name, args), = rec.named("ebm_")
    assert name == GHMC_ENTRY and args[13] == 1 and args[15] is None and args[16] is None


@pytest.mark.parametrize("cls,entry,extra", [(ta.UnderdampedLangevin, BAOAB_ENTRY, {}), (ta.GeneralizedHMC, GHMC_ENTRY, dict(n_leapfrog_steps=2))],
                         ids=["baoab", "ghmc"])
def test_sample_moments_stays_step_by_step(fused_cpu, monkeypatch, mlp_spec_on_cpu, cls, entry, extra):  # noqa: F811
    s, rec, _ = _opted(fused_cpu, cls, mm.mass_of("diag", 5), **extra)
    _route_as_cuda(monkeypatch, s)
    s.fused_mlp = s.fused_mlp_mass = s.fused_mlp_moments = True
    x, mom, p = s.sample_moments(x=torch.randn(16, 5, generator=_gen(1)), n_steps=6, return_velocity=True)
    assert not rec.named("ebm_kinetic_moments") and len(rec.named(entry)) == 6  # the massed chain entry, once per transition
    assert mom.chain_mean.shape == (2, 16, 5)
