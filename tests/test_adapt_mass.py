"""Step-size adaptation under a mass, and warmup(), without a GPU: the cases of adapt_mass_cases.py, the routing with and without the
opt-in `fused_adapt_mass`, the one recorded launch of the massed fused route, the entry's declaration and its refusals in front of
any launch, warmup() against the composition written out with public calls, and the payoff on the badly scaled Gaussian."""

import math
import os
import re

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib, _rng
from torchebm_amd.samplers import adapt
from helpers import fused_cpu  # noqa: F401  (the fixture)
import adapt_mass_cases as amc
import mass_cases as mc
from adapt_mass_cases import CASES, KINDS, MARGIN_BAR, SEED_CAP, case, energy_spec, model_of
from test_adapt import REFUSALS as UNIT_REFUSALS

ENTRY = "ebm_ghmc_adapt_chain_mass_f32"
UNIT_ENTRY = "ebm_ghmc_adapt_chain_f32"
INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------
def test_the_grid():
    assert len(CASES) == 40 and len(set(CASES)) == 40 and len(KINDS) == 7
    assert {c[3] for c in CASES} == {2, 4} and {c[6] for c in CASES} == {"scalar", "diag"}
    assert {c[2] for c in CASES} == {9, 37, 257} and min(c[1] for c in CASES) == 2 and max(c[1] for c in CASES) == 256
    assert SEED_CAP == 200


@pytest.mark.parametrize("kind,dim,n,n_mh,thin,L,form", CASES)
def test_every_case_finds_its_seed(kind, dim, n, n_mh, thin, L, form):
    c = case(kind, dim, n, n_mh, thin, L, form)
    print(f"{kind} dim {dim} n {n} n_mh {n_mh} {form}: {c['seed'] + 1} tries")
    assert c["found"], f"no seed among {SEED_CAP}"
    assert c["ref64"]["margin"] > MARGIN_BAR, (c["seed"], c["ref64"]["margin"])
    assert torch.equal(c["ref32"]["accepted"], c["ref64"]["accepted"])
    assert c["ref32"]["accepted"].shape == c["ref32"]["eps_trace"].shape == (n_mh, n) and c["ref32"]["da"].shape == (3, n)
    assert torch.equal(c["ref32"]["eps_trace"][0], torch.full((n,), amc.f32(c["eps0"])))
    assert not torch.equal(c["ref32"]["da"][0], torch.full((n,), amc.f32(c["eps0"])))  # the controller acted


@pytest.mark.parametrize("kind", KINDS)
def test_every_kind_accepts_and_rejects(kind):
    acc = torch.cat([case(*c)["ref32"]["accepted"].flatten() for c in CASES if c[0] == kind])
    assert acc.any() and (~acc).any()


def test_the_restatement_at_mass_one_is_the_unit_mass_restatement():
    """Identity (a) on the restatement itself, and identity (b): frozen, it is mass_cases.restate_ghmc."""
    import adapt_cases as ac

    spec, n, dim, n_mh, L = energy_spec("double_well", 5), 9, 5, 5, 3
    g = _gen(3)
    x0, v0 = torch.randn(n, dim, generator=g), torch.randn(n, dim, generator=g)
    z, u = torch.randn(n_mh, n, dim, generator=g), torch.rand(n_mh, n, generator=g)
    want = ac.restate(amc.oracle_of(spec), x0, v0, z, u, 0.1, L, amc.GAMMA, amc.TEMP)
    for mass in (1.0, torch.ones(dim)):
        got = amc.restate(amc.oracle_of(spec), x0, v0, z, u, 0.1, L, amc.GAMMA, amc.TEMP, mass)
        for key in ("x", "v", "da", "accepted", "eps_trace", "alpha_mean"):
            assert torch.equal(got[key], want[key]), key
    mass = mc.diag_mass(dim)
    eps = amc.f32(0.07)
    da = torch.stack((torch.full((n,), eps), torch.zeros(n), torch.zeros(n)))
    got = amc.restate(amc.oracle_of(spec), x0, v0, z, u, 0.5, L, math.inf, 1.0, mass, n_adapt=0, da=da)
    want = mc.restate_ghmc(amc.oracle_of(spec), x0, v0, z, u, eps, L, math.inf, 1.0, mass)
    assert torch.equal(got["accepted"], want["accepted"]) and want["accepted"].any()
    assert torch.allclose(got["x"], want["x"], rtol=1e-5, atol=1e-6)  # ((eps p) / m there, (eps / m) p here: a rounding apart)


# ---------------------------------------------------------------------------------
# routing
# ---------------------------------------------------------------------------------
class AsCuda:  # what the routing reads of a state, with no GPU at hand
    def __init__(self, dim, dtype=torch.float32, ndim=2):
        self.is_cuda, self.dtype, self.ndim, self.shape, self.device = True, dtype, ndim, (8, dim), torch.device("cpu")


def _massed(cls, mass, model=None, **kw):
    kw = {**dict(step_size=0.05, n_leapfrog_steps=2), **kw}
    return cls(model or ta.DoubleWellModel(), mass=mass, **kw)


@pytest.mark.parametrize("cls", [ta.GeneralizedHMC, ta.HamiltonianMonteCarlo])
def test_the_opt_in_routes_a_massed_sampler_to_the_new_entry(cls):
    assert cls.fused_adapt_mass is False
    for mass in (2.0, torch.tensor([1.0, 2.0, 0.5, 4.0, 1.0, 1.0, 3.0, 0.25])):
        s = _massed(cls, mass)
        assert adapt.adapt_route(s, AsCuda(8), 1.0) == ("eager", None)  # off, the default
        s.fused_adapt_mass = True
        route, spec = adapt.adapt_route(s, AsCuda(8), 1.0)
        assert route == "fused_mass" and spec is not None and spec.kind == _lib.ENERGY_DOUBLE_WELL
        assert adapt.adapt_route(s, torch.zeros(8, 8), 1.0) == ("eager", None)  # the CPU
        assert adapt.adapt_route(s, AsCuda(8, torch.float64), 1.0) == ("eager", None)
    wide = _massed(cls, 2.0)
    sched = _massed(cls, 2.0, step_size=ta.core.schedules.LinearScheduler(0.3, 0.1, 10))
    mlp = _massed(cls, 2.0, model=ta.MLPEnergy(8, 64), step_size=0.01)
    for s in (wide, sched, mlp):
        s.fused_adapt_mass = True
    assert adapt.adapt_route(wide, AsCuda(300), 1.0) == ("eager", None)
    assert adapt.adapt_route(wide, AsCuda(256), 1.0)[0] == "fused_mass"
    assert adapt.adapt_route(sched, AsCuda(8), 1.0) == ("eager", None)
    assert adapt.adapt_route(mlp, AsCuda(8), 1.0) == ("eager", None)
    # the unit-mass route does not read the opt-in
    unit = cls(ta.DoubleWellModel(), step_size=0.05, n_leapfrog_steps=2)
    unit.fused_adapt_mass = True
    assert adapt.adapt_route(unit, AsCuda(8), 1.0)[0] == "fused"


@pytest.mark.parametrize("which", ["ghmc", "hmc"])
@pytest.mark.parametrize("form", ["scalar", "diag"])
def test_the_fused_route_is_one_recorded_launch(fused_cpu, monkeypatch, which, form):  # noqa: F811
    make, rec, _ = fused_cpu
    reserved = []
    monkeypatch.setattr(_rng, "reserve", lambda generator, device, n_steps: reserved.append(n_steps) or (7, 11))
    mass = 0.37 if form == "scalar" else torch.tensor([1.0, 2.0, 0.5, 4.0])
    if which == "ghmc":
        s, gamma, temp = make(ta.GeneralizedHMC, step_size=0.05, n_leapfrog_steps=3, friction=1.5, temperature=0.8, mass=mass), 1.5, 0.8
    else:
        s, gamma, temp = make(ta.HamiltonianMonteCarlo, step_size=0.05, n_leapfrog_steps=3, mass=mass), math.inf, 1.0
    x0 = torch.randn(16, 4, generator=_gen(1))
    keep = x0.clone()
    # off: the eager route, no launch
    r = s.adapt_step_size(x=x0, n_steps=5, apply=False, generator=_gen(2))
    assert rec.calls == [] and reserved == []
    s.fused_adapt_mass = True
    r = s.adapt_step_size(x=x0, n_steps=5, target_accept=0.7, bounds=(1e-4, 10.0), apply=False)
    assert reserved == [2 * 5 + 1]
    assert [name for name, _ in rec.calls] == [ENTRY]
    a = rec.calls[0][1]
    assert len(a) == len(_lib._PROTOTYPES[ENTRY][1]) == 32
    assert a[1] == r.x.data_ptr() != x0.data_ptr() and a[2] == r.velocity.data_ptr() and torch.equal(x0, keep)
    assert tuple(a[3:14]) == (16, 4, 5, 3, 0.05, 0.7, math.log(10.0 * 0.05), 1e-4, 10.0, 5, _lib.DA_INIT)
    assert a[14] == r.da.data_ptr() and a[15] is not None and a[16] is None and a[17] == r.acceptance.data_ptr()
    assert tuple(a[18:20]) == (gamma, temp)
    if form == "scalar":
        assert tuple(a[20:23]) == (_lib.MASS_SCALAR, 0.37, None)
    else:
        assert tuple(a[20:22]) == (_lib.MASS_DIAG, 0.0) and a[22] is not None
    assert tuple(a[23:]) == (1, 1, None, None, None, None, 7, 11, None)
    # a passed momentum plane is copied and read (draw_v0 = 0)
    rec.calls.clear()
    v0 = torch.ones(16, 4)
    r = s.adapt_step_size(x=x0, n_steps=5, velocity=v0, init_step_size=0.2, apply=False)
    a = rec.calls[0][1]
    assert a[2] == r.velocity.data_ptr() != v0.data_ptr() and torch.equal(v0, torch.ones(16, 4))
    assert a[7] == 0.2 and a[9] == math.log(2.0) and a[23] == 0 and len(rec.named(ENTRY)) == 1 and len(rec.named(UNIT_ENTRY)) == 0


# ---------------------------------------------------------------------------------
# the entry
# ---------------------------------------------------------------------------------
def _abi_call(desc, *, x=16, v=16, n=4, dim=8, n_mh=3, L=2, eps0=0.1, delta=0.8, mu=0.0, eps_min=1e-6, eps_max=1e3, n_adapt=3,
              init_da=1, da=16, table=16, trace=None, alpha=None, gamma=1.0, temp=1.0, mass_kind=_lib.MASS_SCALAR, mass_scalar=2.0,
              mass_diag=None, thin=1, traj=None, mask=None):
    _lib.call(ENTRY, desc, x, v, n, dim, n_mh, L, eps0, delta, mu, eps_min, eps_max, n_adapt, init_da, da, table, trace, alpha, gamma, temp,
              mass_kind, mass_scalar, mass_diag, 0, thin, traj, mask, None, None, 0, 0, None)


# the unit-mass adapt entry's refusals in its order, then check_chain_mass's
REFUSALS = list(UNIT_REFUSALS) + [
    (dict(mass_kind=_lib.MASS_NONE), ValueError, "mass_kind=0"),
    (dict(mass_kind=3), ValueError, "mass_kind=3"),
    (dict(mass_kind=_lib.MASS_DIAG, mass_diag=None), ValueError, "mass_diag is NULL"),
    (dict(mass_scalar=0.0), ValueError, "mass_scalar=0 "),
    (dict(mass_scalar=-1.0), ValueError, "mass_scalar=-1 "),
    (dict(mass_scalar=math.inf), ValueError, "mass_scalar=inf"),
    (dict(mass_scalar=float("nan")), ValueError, "mass_scalar=nan"),
]


def test_abi_refusals_need_no_gpu():
    """Every refusal comes in front of any launch (the pointers below are never dereferenced)."""
    desc = _lib.EnergyDesc()
    desc.kind = _lib.ENERGY_DOUBLE_WELL
    for kw, exc, match in REFUSALS:
        with pytest.raises(exc, match=match):
            _abi_call(desc, **kw)
    with pytest.raises(ValueError, match="energy descriptor is NULL"):
        _abi_call(None)
    desc.kind, desc.dev0 = _lib.ENERGY_MLP, 16
    with pytest.raises(RuntimeError, match=r"code -2.*no generalized-HMC kernel"):  # EBM_EKIND
        _abi_call(desc)
    desc.kind = _lib.ENERGY_DOUBLE_WELL
    # the order: the adaptation's refusals stand in front of the mass's
    with pytest.raises(ValueError, match="mu=inf"):
        _abi_call(desc, mu=math.inf, mass_kind=_lib.MASS_NONE)
    _abi_call(desc, n=0)  # an empty call returns in front of any launch
    _abi_call(desc, n=0, mass_kind=_lib.MASS_DIAG, mass_diag=16, mass_scalar=0.0)  # (the scalar is not read with a diagonal)
    for kw, match in ((dict(da=None), "da pointer is NULL"), (dict(mass_kind=_lib.MASS_NONE), "mass_kind=0"),
                      (dict(mass_scalar=0.0), "mass_scalar=0 ")):
        with pytest.raises(ValueError, match=match):
            _abi_call(desc, n=0, **kw)  # ... but the refusals come first


def test_the_entry_is_exported_and_declared():
    """Fails without the feature."""
    texts = {}
    for name in ("ebm_hip.h", "ebm_hip_adapt.h", "ebm_hip_adapt_mass.h"):
        with open(os.path.join(INCLUDE, name)) as fh:
            texts[name] = fh.read()
    companion = texts["ebm_hip_adapt_mass.h"]
    assert '#include "ebm_hip_adapt.h"' in companion
    assert re.findall(r"EBM_API\s+int\s+(ebm_\w+)\s*\(", companion) == list(_lib.EXPORTS_ADAPT_MASS) == [ENTRY]

    def params(text, name):
        m = re.search(r"EBM_API\s+int\s+" + name + r"\s*\(([^)]*)\)", text)
        assert m, name
        return re.sub(r"\s+", " ", m.group(1)).strip()

    three = "double temperature, int32_t mass_kind, double mass_scalar, const float* mass_diag, "
    assert params(companion, ENTRY) == params(texts["ebm_hip_adapt.h"], UNIT_ENTRY).replace("double temperature, ", three)
    assert three in params(texts["ebm_hip.h"], "ebm_ghmc_chain_mass_f32")  # where the massed entries put them
    proto, unit = _lib._PROTOTYPES[ENTRY][1], _lib._PROTOTYPES[UNIT_ENTRY][1]
    assert proto == unit[:20] + [_lib._i32, _lib._d, _lib._p] + unit[20:] and len(proto) == 32
    assert hasattr(_lib.lib(), ENTRY)
    assert ENTRY not in _lib.EXPORTS and ENTRY not in _lib.EXPORTS_ADAPT and ENTRY not in _lib.EXPORTS_MASS_MLP
    assert _lib.ABI_VERSION == 9 and _lib.lib().ebm_version() == 9 and len(_lib.EXPORTS) == 58
    assert _lib.EXPORTS_ADAPT == (UNIT_ENTRY,)
    for text in ("drift_j   = eps / m_safe_j", "refresh_j = c2 * m_sqrt_j", "p ~ N(0, T m)", "EBM_MASS_NONE"):  # the contract
        assert text in companion


# ---------------------------------------------------------------------------------
# warmup()
# ---------------------------------------------------------------------------------
def _written_out(s, x0, windows, final, seed, regularize=True, **kw):
    """warmup() with public calls: adapt_step_size per window under the current mass, the pooled variance, the shrinkage, 1 / var."""
    g = _gen(seed)
    x, eps, n = x0, None, x0.shape[0]
    prev = torch.ones(x0.shape[1]) if s.mass is None else (torch.full((x0.shape[1],), s.mass) if isinstance(s.mass, float) else s.mass)
    eps_list, acc_list, masses = [], [], []
    for i, w in enumerate(list(windows) + [final]):
        r = s.adapt_step_size(x=x, n_steps=w, velocity=None, init_step_size=eps, generator=g, apply=False, **kw)
        x, eps = r.x, float(r.step_size)
        eps_list.append(r.step_size)
        acc_list.append(r.acceptance.mean())
        if i < len(windows):
            var = x.reshape(-1, x.shape[-1]).var(0)
            if regularize:
                var = n / (n + 5.0) * var + 1e-3 * (5.0 / (n + 5.0))
            prev = torch.where(torch.isfinite(var) & (var > 0), 1.0 / var, prev)
            masses.append(prev)
            s.mass = prev
    return x, eps_list, acc_list, masses, g


def _make(cls, kind, dim, mass=None):
    spec = energy_spec(kind, dim)
    kw = dict(friction=1.5, temperature=0.8) if cls is ta.GeneralizedHMC else {}
    return cls(model_of(spec), step_size=2.0 * mc.ghmc_cases.step_size(kind, dim), n_leapfrog_steps=2, mass=mass, **kw)


@pytest.mark.parametrize("cls", [ta.GeneralizedHMC, ta.HamiltonianMonteCarlo])
@pytest.mark.parametrize("kind,dim", [("double_well", 2), ("double_well", 5), ("gaussian", 2), ("gaussian", 5)])
@pytest.mark.parametrize("regularize", [True, False])
def test_warmup_is_the_composition_written_out(cls, kind, dim, regularize):
    x0 = torch.randn(9, dim, generator=_gen(3))
    keep = x0.clone()
    want_x, want_eps, want_acc, want_masses, g_want = _written_out(_make(cls, kind, dim), x0, (3, 4), 3, 17, regularize, target_accept=0.7)
    s = _make(cls, kind, dim)
    eps_before = s.get_scheduled_value("step_size")
    g = _gen(17)
    w = s.warmup(x=x0, windows=(3, 4), final_steps=3, target_accept=0.7, regularize=regularize, generator=g, apply=False)
    assert isinstance(w, ta.samplers.Warmup) and torch.equal(x0, keep)
    assert torch.equal(w.x, want_x) and torch.equal(w.step_size, want_eps[-1]) and w.step_size.ndim == 0
    assert torch.equal(w.mass, want_masses[-1]) and w.mass.shape == (dim,) and w.mass.dtype == torch.float32
    assert len(w.step_sizes) == len(w.acceptances) == 3 and len(w.masses) == 2
    for got, want in zip(w.step_sizes + w.acceptances + w.masses, want_eps + want_acc + want_masses):
        assert torch.equal(got, want)
    assert torch.equal(g.get_state(), g_want.get_state())  # the generator ends where the composition's ends
    assert not torch.equal(w.masses[0], w.masses[1]) and not torch.equal(w.step_sizes[0], w.step_sizes[2])
    # apply=False left the sampler as it was
    assert s.mass is None and s.get_scheduled_value("step_size") == eps_before and "fused_adapt_mass" not in vars(s)


def test_warmup_starts_from_the_samplers_own_mass_and_passes_the_constants():
    x0 = torch.randn(9, 5, generator=_gen(3))
    for mass in (0.37, mc.diag_mass(5)):
        kw = dict(t0=5.0, gamma=0.1, kappa=0.6, mu_factor=4.0, bounds=(1e-3, 2.0))
        want = _written_out(_make(ta.GeneralizedHMC, "double_well", 5, mass), x0, (3,), 2, 5, **kw)
        s = _make(ta.GeneralizedHMC, "double_well", 5, mass)
        w = s.warmup(x=x0, windows=(3,), final_steps=2, generator=_gen(5), apply=False, **kw)
        assert torch.equal(w.x, want[0]) and torch.equal(w.mass, want[3][-1]) and torch.equal(w.step_size, want[1][-1])
        assert (s.mass == mass) if isinstance(mass, float) else torch.equal(s.mass, mass)
    with pytest.raises(TypeError, match="unexpected keyword"):
        s.warmup(x=x0, n_steps=3)
    # no mass window: the terminal window alone, under the sampler's own mass
    s = _make(ta.GeneralizedHMC, "double_well", 5, 0.37)
    w = s.warmup(x=x0, windows=(), final_steps=3, generator=_gen(5), apply=False)
    r = s.adapt_step_size(x=x0, n_steps=3, generator=_gen(5), apply=False)
    assert torch.equal(w.x, r.x) and torch.equal(w.step_size, r.step_size) and w.masses == []
    assert torch.equal(w.mass, torch.full((5,), 0.37))


def test_a_coordinate_without_a_variance_keeps_its_mass():
    from torchebm_amd.samplers.warmup import mass_from_positions

    x = torch.randn(64, 4, generator=_gen(0))
    x[:, 1] = float("nan")
    x[:, 3] = 2.5  # zero variance: kept only without the shrinkage, which makes it positive
    prev = torch.tensor([3.0, 5.0, 7.0, 9.0])
    raw = mass_from_positions(x, prev, regularize=False)
    assert raw[1] == 5.0 and raw[3] == 9.0 and torch.equal(raw[[0, 2]], 1.0 / x[:, [0, 2]].var(0))
    reg = mass_from_positions(x, prev, regularize=True)
    assert reg[1] == 5.0 and math.isclose(reg[3].item(), 1.0 / (1e-3 * 5.0 / 69.0), rel_tol=1e-6)
    assert torch.allclose(reg[[0, 2]], 1.0 / (64.0 / 69.0 * x[:, [0, 2]].var(0) + 1e-3 * 5.0 / 69.0), rtol=1e-6)
    # through warmup(): a chain ensemble whose one coordinate is NaN keeps that coordinate's mass through every window
    s = _make(ta.GeneralizedHMC, "double_well", 4, torch.tensor([3.0, 5.0, 7.0, 9.0]))
    x0 = torch.randn(16, 4, generator=_gen(1))
    x0[:, 2] = float("nan")
    w = s.warmup(x=x0, windows=(2, 2), final_steps=2, generator=_gen(2), apply=False)
    assert all(m[2] == 7.0 for m in w.masses) and w.mass[2] == 7.0 and torch.isfinite(w.mass).all()


@pytest.mark.parametrize("cls", [ta.GeneralizedHMC, ta.HamiltonianMonteCarlo])
def test_apply_sets_step_size_and_mass(cls):
    s = _make(cls, "gaussian", 5)
    x0 = torch.randn(32, 5, generator=_gen(3))
    w = s.warmup(x=x0, windows=(4, 4), final_steps=4, generator=_gen(4))
    assert s.get_scheduled_value("step_size") == float(w.step_size) and s.schedulers["step_size"].is_constant()
    assert torch.equal(s.mass, w.mass) and s.mass.ndim == 1 and s.mass.device == s.device
    assert cls.fused_adapt_mass is False and "fused_adapt_mass" not in vars(s)
    out = s.sample(x=w.x, n_steps=3, generator=_gen(5))  # the sampler runs on with what warmup set
    assert out.shape == (32, 5) and torch.isfinite(out).all()


def test_fewer_than_two_rows_raise():
    s = _make(ta.GeneralizedHMC, "double_well", 3)
    with pytest.raises(ValueError, match="at least 2 rows"):
        s.warmup(x=torch.zeros(1, 3))
    with pytest.raises(ValueError, match="at least 2 rows"):
        s.warmup(dim=3, n_samples=1)
    with pytest.raises(ValueError, match="dim must be provided"):
        s.warmup()
    assert s.mass is None


# ---------------------------------------------------------------------------------
# the payoff
# ---------------------------------------------------------------------------------
def test_the_payoff_on_the_badly_scaled_gaussian():
    """sigma = (1, 0.1, 0.01), 4096 chains started from the target law (so every window's final positions are exact draws): after
    warmup() every m_j sigma_j^2 lies within exp(+-4.5 sqrt(2 / (N - 1))) of the regularised expectation, and the adapted step size
    is larger than the unit-mass adapted step size of the same sampler."""
    n, sigma = mc.PAYOFF_N, mc.PAYOFF_SIGMA
    x0 = mc.payoff_start()
    make = lambda: ta.GeneralizedHMC(mc.payoff_model(), step_size=0.005, n_leapfrog_steps=4, friction=math.inf)  # noqa: E731
    s = make()
    w = s.warmup(x=x0, windows=(20, 20), final_steps=30, generator=_gen(0))
    ratio = w.mass.double() * torch.tensor(sigma, dtype=torch.float64) ** 2
    want, margin = amc.payoff_expectation(sigma, n), amc.payoff_margin(n)
    unit = make().adapt_step_size(x=x0, n_steps=70, generator=_gen(0), apply=False)
    print(f"m sigma^2 = {ratio.tolist()}, expected {want.tolist()}, factor {margin:.4f}; step size {float(w.step_size):.4f} against "
          f"{float(unit.step_size):.5f} at unit mass; acceptances {[round(float(a), 3) for a in w.acceptances]}")
    assert math.isclose(margin, math.exp(4.5 * math.sqrt(2.0 / 4095.0)), rel_tol=1e-12)
    assert bool((ratio < want * margin).all()) and bool((ratio > want / margin).all())
    assert float(w.step_size) > float(unit.step_size)
    assert torch.equal(s.mass, w.mass) and s.get_scheduled_value("step_size") == float(w.step_size)
