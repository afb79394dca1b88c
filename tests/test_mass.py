"""UnderdampedLangevin and GeneralizedHMC with a scalar or diagonal mass, without a GPU: the eager routes against the independent
restatements of mass_cases.py on the same generator draws, a run cut in two, mass 1 against no mass, friction = inf against
HamiltonianMonteCarlo with the same mass, the decisions of every GPU case, the laws on a quadratic, what the mass buys on a badly
scaled Gaussian, validation and routing, the one recorded launch of the fused route, sample_moments, ChainMoments.diagonal_mass
and the refusals the two entries make in front of any launch."""

import math

import pytest
import torch

import torchebm_amd as ta
from torchebm_amd import _lib, _rng
from helpers import fused_cpu  # noqa: F401  (the fixture)
import mass_cases as mc
from mass_cases import GAMMA, TEMP, energy_spec, model_of, oracle_of

BAOAB_ENTRY, GHMC_ENTRY = "ebm_kinetic_chain_mass_f32", "ebm_ghmc_chain_mass_f32"
FORMS = ("scalar", "diag")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _baoab(spec, h, mass, **kw):
    return ta.UnderdampedLangevin(model_of(spec), step_size=h, friction=GAMMA, temperature=TEMP, mass=mass, **kw)


def _ghmc(spec, eps, L, mass, gamma=GAMMA, temp=TEMP):
    return ta.GeneralizedHMC(model_of(spec), step_size=eps, n_leapfrog_steps=L, friction=gamma, temperature=temp, mass=mass)


def _replay_baoab(seed, n, dim, k, with_v0=True):
    g = _gen(seed)
    xi0 = torch.randn(n, dim, generator=g) if with_v0 else None
    return xi0, torch.stack([torch.randn(n, dim, generator=g) for _ in range(k)])


def _replay_ghmc(seed, n, dim, n_mh, with_v0=True):
    g = _gen(seed)
    xi0 = torch.randn(n, dim, generator=g) if with_v0 else None
    z, u = [], []
    for _ in range(n_mh):
        z.append(torch.randn(n, dim, generator=g))
        u.append(torch.rand(n, generator=g))
    return xi0, torch.stack(z), torch.stack(u)


# ---------------------------------------------------------------------------------
# the eager routes against the restatements
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind,dim", [("double_well", 2), ("double_well", 5), ("harmonic", 5), ("gaussian", 5)])
def test_eager_baoab_equals_the_restatement_bit_for_bit(kind, dim, form):
    spec, mass, n, k = energy_spec(kind, dim), mc.mass_of(form, dim), 9, 11
    h = 2.0 * mc.baoab_step(kind, mass)
    x0 = torch.randn(n, dim, generator=_gen(3))
    xi0, noise = _replay_baoab(11, n, dim, k)
    s = _baoab(spec, h, mass)
    for thin in (1, 3):
        want = mc.restate_baoab(oracle_of(spec), x0, None, noise, h, GAMMA, TEMP, mass, thin, xi0=xi0)
        x, p = s.sample(x=x0, n_steps=k, return_velocity=True, generator=_gen(11))
        assert torch.equal(x, want["x"]) and torch.equal(p, want["v"])
        traj = s.sample(x=x0, n_steps=k, thin=thin, return_trajectory=True, generator=_gen(11))
        assert traj.shape == (n, k // thin, dim) and torch.equal(traj, want["traj"])
    assert not torch.equal(want["x"], x0)
    # a given start momentum is used as it is, and the caller's tensors, the mass included, stay
    p0 = mc.start_momentum(mass, torch.randn(n, dim, generator=_gen(4)))
    _, noise = _replay_baoab(11, n, dim, k, with_v0=False)
    want = mc.restate_baoab(oracle_of(spec), x0, p0, noise, h, GAMMA, TEMP, mass)
    keep = (x0.clone(), p0.clone(), mass if form == "scalar" else mass.clone())
    x, p = s.sample(x=x0, n_steps=k, velocity=p0, return_velocity=True, generator=_gen(11))
    assert torch.equal(x, want["x"]) and torch.equal(p, want["v"])
    assert torch.equal(x0, keep[0]) and torch.equal(p0, keep[1]) and (form == "scalar" or torch.equal(mass, keep[2]))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("kind,dim", [("double_well", 2), ("double_well", 5), ("harmonic", 5), ("gaussian", 5)])
def test_eager_ghmc_equals_the_restatement_bit_for_bit(kind, dim, L, form):
    spec, mass, n, n_mh = energy_spec(kind, dim), mc.mass_of(form, dim), 9, 11
    eps = 2.0 * mc.ghmc_step(kind, dim, mass)
    x0 = torch.randn(n, dim, generator=_gen(3))
    xi0, z, u = _replay_ghmc(11, n, dim, n_mh)
    s = _ghmc(spec, eps, L, mass)
    for thin in (1, 3):
        want = mc.restate_ghmc(oracle_of(spec), x0, None, z, u, eps, L, GAMMA, TEMP, mass, torch.float32, thin, xi0=xi0)
        x, p = s.sample(x=x0, n_steps=n_mh, return_velocity=True, generator=_gen(11))
        assert torch.equal(x, want["x"]) and torch.equal(p, want["v"])
        traj, diag = s.sample(x=x0, n_steps=n_mh, thin=thin, return_trajectory=True, return_diagnostics=True, generator=_gen(11))
        assert torch.equal(traj, want["traj"])
        assert torch.equal(diag["acceptance_rate"], want["accepted"][thin - 1 :: thin][: n_mh // thin].float().mean(dim=1))
    p0 = mc.start_momentum(mass, torch.randn(n, dim, generator=_gen(4)))
    _, z, u = _replay_ghmc(11, n, dim, n_mh, with_v0=False)
    want = mc.restate_ghmc(oracle_of(spec), x0, p0, z, u, eps, L, GAMMA, TEMP, mass)
    x, p = s.sample(x=x0, n_steps=n_mh, velocity=p0, return_velocity=True, generator=_gen(11))
    assert torch.equal(x, want["x"]) and torch.equal(p, want["v"])


def test_the_eager_ghmc_runs_accept_and_reject():
    seen = torch.zeros(2, dtype=torch.bool)
    for form in FORMS:
        spec, mass = energy_spec("double_well", 5), mc.mass_of(form, 5)
        xi0, z, u = _replay_ghmc(11, 9, 5, 11)
        acc = mc.restate_ghmc(oracle_of(spec), torch.randn(9, 5, generator=_gen(3)), None, z, u, 2.0 * mc.ghmc_step("double_well", 5, mass),
                              3, GAMMA, TEMP, mass, xi0=xi0)["accepted"]
        seen |= torch.tensor([bool(acc.any()), bool((~acc).any())])
    assert seen.all()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("sampler", ["baoab", "ghmc"])
def test_a_run_cut_in_two_is_the_uncut_run(sampler, form):
    kind, n, dim, k1, k2 = "gaussian", 9, 5, 4, 7
    spec, mass = energy_spec(kind, dim), mc.mass_of(form, dim)
    s = _baoab(spec, mc.baoab_step(kind, mass), mass) if sampler == "baoab" else _ghmc(spec, 2.0 * mc.ghmc_step(kind, dim, mass), 3, mass)
    x0 = torch.randn(n, dim, generator=_gen(5))
    whole_x, whole_p = s.sample(x=x0, n_steps=k1 + k2, return_velocity=True, generator=_gen(12))
    g = _gen(12)
    x, p = s.sample(x=x0, n_steps=k1, return_velocity=True, generator=g)
    x, p = s.sample(x=x, n_steps=k2, velocity=p, return_velocity=True, reset_schedulers=False, generator=g)
    assert torch.equal(x, whole_x) and torch.equal(p, whole_p)


@pytest.mark.parametrize("kind", ["double_well", "gaussian"])
@pytest.mark.parametrize("sampler", ["baoab", "ghmc"])
def test_mass_one_is_no_mass_bit_for_bit(sampler, kind):
    n, dim, k = 9, 5, 11
    spec = energy_spec(kind, dim)
    x0 = torch.randn(n, dim, generator=_gen(6))
    make = (lambda m: _baoab(spec, 2.0 * mc.kinetic_cases.STEP[kind], m)) if sampler == "baoab" else (
        lambda m: _ghmc(spec, 2.0 * mc.ghmc_cases.step_size(kind, dim), 3, m))
    want = make(None).sample(x=x0, n_steps=k, thin=2, return_trajectory=True, return_diagnostics=True, return_velocity=True, generator=_gen(14))
    for mass in (1.0, torch.ones(dim)):
        got = make(mass).sample(x=x0, n_steps=k, thin=2, return_trajectory=True, return_diagnostics=True, return_velocity=True,
                                generator=_gen(14))
        assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])
        assert torch.equal(got[1]["kinetic_temperature"], want[1]["kinetic_temperature"])
    assert not torch.equal(want[0][:, -1], x0)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", ["double_well", "gaussian"])
def test_infinite_friction_is_hamiltonian_monte_carlo_with_the_mass(kind, form):
    """friction = inf, T = 1 and a start momentum passed: the draw orders coincide and the runs are equal bit for bit, as
    test_ghmc.py's test_infinite_friction_is_hamiltonian_monte_carlo has it at unit mass."""
    n, dim, n_mh, L = 9, 5, 11, 3
    spec, mass = energy_spec(kind, dim), mc.mass_of(form, dim)
    eps = 2.0 * mc.ghmc_step(kind, dim, mass)
    x0 = torch.randn(n, dim, generator=_gen(6))
    hmc = ta.HamiltonianMonteCarlo(model_of(spec), step_size=eps, n_leapfrog_steps=L, mass=mass)
    want, want_diag = hmc.sample(x=x0, n_steps=n_mh, return_diagnostics=True, generator=_gen(13))
    s = _ghmc(spec, eps, L, mass, gamma=math.inf, temp=1.0)
    got, diag = s.sample(x=x0, n_steps=n_mh, velocity=torch.zeros(n, dim), return_diagnostics=True, generator=_gen(13))
    assert torch.equal(got, want) and torch.equal(diag["acceptance_rate"], want_diag["acceptance_rate"])
    assert 0.0 < diag["acceptance_rate"].mean() < 1.0 and not torch.equal(got, x0)


# ---------------------------------------------------------------------------------
# the GPU cases
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dim,n,n_mh,thin,L,form", mc.GHMC_CASES)
def test_every_gpu_case_has_a_seed_within_the_cap(kind, dim, n, n_mh, thin, L, form):
    c = mc.ghmc_case(kind, dim, n, n_mh, thin, L, form)
    assert c["found"] and c["seed"] < mc.SEED_CAP, (c["seed"], c["ref64"]["margin"])
    assert c["ref64"]["margin"] > mc.MARGIN_BAR and torch.equal(c["ref32"]["accepted"], c["ref64"]["accepted"])
    assert c["ref32"]["accepted"].shape == (n_mh, n) and c["ref32"]["traj"].shape == (n, n_mh // thin, dim)


def test_the_cases_cover_the_shapes_and_both_forms():
    for cases, per in ((mc.BAOAB_EXACT + mc.BAOAB_COUPLED, 5), (mc.GHMC_CASES, 6)):
        assert 18 <= len(cases) <= 24
        assert {c[1] for c in cases} == {2, 5, 12, 32, 64, 100, 256} and {c[2] for c in cases} == {9, 37, 257}
        assert {c[0] for c in cases} == set(mc.kinetic_cases.STEP)
        for dim in (5, 12, 100):  # the masked rows see a diagonal mass
            assert any(c[1] == dim and c[per] == "diag" for c in cases)
        assert {(c[0], c[per]) for c in cases} >= {(kind, form) for kind in mc.kinetic_cases.STEP for form in FORMS}
    assert {(c[3], c[4]) for c in mc.BAOAB_EXACT + mc.BAOAB_COUPLED} == {(1, 1), (4, 2), (11, 3)}
    assert {(c[3], c[4]) for c in mc.GHMC_CASES} == {(1, 1), (4, 2), (6, 3)} and {c[5] for c in mc.GHMC_CASES} == {1, 3}
    acc = torch.cat([mc.ghmc_case(*c)["ref32"]["accepted"].flatten() for c in mc.GHMC_CASES])
    print("rejected", int((~acc).sum()), "of", acc.numel())
    assert acc.any() and (~acc).any()
    d = mc.diag_mass(100)
    assert 0.5 <= float(d.min()) < 0.6 and 3.5 < float(d.max()) <= 4.0 and mc.SCALAR_MASS == 0.37


# ---------------------------------------------------------------------------------
# the laws and the payoff
# ---------------------------------------------------------------------------------
def test_the_baoab_law_with_a_mass():
    """var(x) k / T = 1 and var(p) / (T m) = 1 - h^2 k / (4 m) = (0.9775, 0.91, 0.91, 0.64): the unit-mass law in x sqrt(m).  (An
    fp64 run of the recurrence gave deviations of at most 0.012 and 0.019 against the bar 0.0497.)"""
    s = ta.UnderdampedLangevin(mc.law_model(), step_size=mc.LAW_STEP, friction=mc.LAW_GAMMA_BAOAB, temperature=mc.LAW_TEMP,
                               mass=torch.tensor(mc.LAW_MASS))
    x, diag, p = s.sample(x=mc.law_start(), n_steps=mc.LAW_STEPS, return_diagnostics=True, return_velocity=True, generator=_gen(mc.LAW_SEED))
    mc.check_law(x, p, baoab=True)
    want = (p.double().square() / torch.tensor(mc.LAW_MASS, dtype=torch.float64)).mean().item()
    assert abs(diag["kinetic_temperature"].item() - want) < 1e-5  # the mean of p^2 / m


def test_the_ghmc_law_with_a_mass():
    s = ta.GeneralizedHMC(mc.law_model(), step_size=mc.LAW_STEP, n_leapfrog_steps=1, friction=mc.LAW_GAMMA_GHMC, temperature=mc.LAW_TEMP,
                          mass=torch.tensor(mc.LAW_MASS))
    x, diag, p = s.sample(x=mc.law_start(), n_steps=mc.LAW_STEPS, thin=mc.LAW_STEPS // 4, return_diagnostics=True, return_velocity=True,
                          generator=_gen(mc.LAW_SEED))
    mc.check_law(x, p, baoab=False)
    print("acceptance", diag["acceptance_rate"].mean().item(), "kinetic_temperature", diag["kinetic_temperature"].item())
    assert abs(diag["kinetic_temperature"].item() / mc.LAW_TEMP - 1.0) < mc.kinetic_cases.law_bar(mc.LAW_N)


def test_the_payoff_on_a_badly_scaled_gaussian():
    """sigma = (1, 0.1, 0.01), HMC transitions with L = 1 (friction = inf), 4096 chains from the law, 50 transitions.  Unit mass:
    the stiff coordinate forbids more than eps = 0.01 and the slow one keeps (1 - eps^2 / 2)^50 = 0.9975 of its start.  With the
    mass 1 / var of a pilot's moments and eps = 1 every coordinate is of unit scale: (1 - 1 / 2)^50 = 0.  Sampling error 0.016."""
    model, x0 = mc.payoff_model(), mc.payoff_start()
    hmc = lambda eps, mass: ta.GeneralizedHMC(model, step_size=eps, n_leapfrog_steps=1, friction=math.inf, mass=mass)  # noqa: E731
    plain = hmc(0.01, None).sample(x=x0, n_steps=mc.PAYOFF_STEPS, generator=_gen(1))
    _, pilot = hmc(0.01, None).sample_moments(x=x0, n_steps=8, generator=_gen(2))
    mass = pilot.diagonal_mass()
    assert mass.dtype == torch.float32 and mass.shape == (3,)
    assert torch.allclose(mass, 1.0 / torch.tensor(mc.PAYOFF_SIGMA) ** 2, rtol=0.1)
    x, diag = hmc(1.0, mass).sample(x=x0, n_steps=mc.PAYOFF_STEPS, return_diagnostics=True, generator=_gen(1))
    slow, fast = mc.slow_correlation(x0, plain), mc.slow_correlation(x0, x)
    print(f"slow-coordinate correlation after {mc.PAYOFF_STEPS} transitions: {slow:.4f} at unit mass, {fast:.4f} with the mass; "
          f"acceptance {diag['acceptance_rate'].mean().item():.3f}")
    assert slow > 0.9 and abs(fast) < 0.1
    assert abs(x[:, 2].double().std().item() / mc.PAYOFF_SIGMA[2] - 1.0) < 0.1  # the stiff coordinate keeps its law at eps = 1


# ---------------------------------------------------------------------------------
# the sampler's surface
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [ta.UnderdampedLangevin, ta.GeneralizedHMC])
def test_validation(cls):
    m = ta.DoubleWellModel()
    for bad in (0.0, -1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="mass must be positive and finite"):
            cls(m, mass=bad)
    with pytest.raises(ValueError, match="1-D tensor"):
        cls(m, mass=torch.ones(2, 2))
    with pytest.raises(ValueError, match="mass must be None, a float or a 1-D tensor"):
        cls(m, mass="heavy")
    assert cls(m).mass is None and cls(m, mass=2).mass == 2.0 and isinstance(cls(m, mass=2).mass, float)
    s = cls(m, mass=torch.ones(3))
    with pytest.raises(ValueError, match="mass tensor must have 2 entries, got 3"):
        s.sample(x=torch.zeros(4, 2), n_steps=1)
    assert s.sample(x=torch.zeros(4, 3), n_steps=2, generator=_gen(1)).shape == (4, 3)
    import inspect

    assert list(inspect.signature(cls.__init__).parameters)[-1] == "mass"  # the keyword is appended last


class AsCuda:  # what _route reads of a state, with no GPU at hand
    def __init__(self, dim, dtype=torch.float32, ndim=2):
        self.is_cuda, self.dtype, self.ndim, self.shape, self.device = True, dtype, ndim, (8, dim), torch.device("cpu")


@pytest.mark.parametrize("cls", [ta.UnderdampedLangevin, ta.GeneralizedHMC])
def test_routing(cls):
    for mass in (0.37, torch.ones(8)):
        s = cls(ta.DoubleWellModel(), step_size=0.05, mass=mass)
        assert s._route(torch.zeros(3, 8)) == ("eager", None)
        assert s._route(AsCuda(8))[0] == s._route(AsCuda(256))[0] == s._route(AsCuda(2))[0] == "fused_mass"
        assert s._route(AsCuda(300))[0] == "eager" and s._route(AsCuda(8, torch.float64))[0] == "eager" and s._route(AsCuda(8, ndim=3))[0] == "eager"
        sched = cls(ta.HarmonicModel(k=4.0), step_size=ta.core.schedules.LinearScheduler(0.3, 0.1, 10), mass=mass)
        assert sched._route(AsCuda(8))[0] == "eager"
        mlp = cls(ta.MLPEnergy(8, 64), step_size=0.01, mass=mass)
        assert mlp._route(AsCuda(8))[0] == "eager"
        mlp.fused_mlp = True  # opted in or not: no mass on the MLP walks
        assert mlp._route(AsCuda(8))[0] == "eager"
    # without a mass: what it returned before
    assert cls(ta.DoubleWellModel(), step_size=0.05)._route(AsCuda(8))[0] == "fused"


def _massed(fused_cpu, monkeypatch, cls, mass, **kw):  # noqa: F811
    make, rec, _ = fused_cpu
    s = make(cls, step_size=0.05, friction=1.5, temperature=0.8, mass=mass, **kw)
    spec = s.model.fused_spec()
    monkeypatch.setattr(s, "_route", lambda x, model_kwargs: ("fused_mass", spec))
    return s, rec


@pytest.mark.parametrize("form", FORMS)
def test_the_fused_baoab_route_is_one_recorded_launch(fused_cpu, monkeypatch, form):  # noqa: F811
    reserved = []
    mass = 0.37 if form == "scalar" else mc.diag_mass(4)
    s, rec = _massed(fused_cpu, monkeypatch, ta.UnderdampedLangevin, mass)
    monkeypatch.setattr(_rng, "reserve", lambda generator, device, n_steps: reserved.append(n_steps) or (7, 11))
    x0 = torch.randn(16, 4, generator=_gen(1))
    keep = x0.clone()
    x, p = s.sample(x=x0, n_steps=5, return_velocity=True)
    assert reserved == [5 + 1] and [name for name, _ in rec.calls] == [BAOAB_ENTRY]
    args = rec.calls[0][1]
    assert args[1] == x.data_ptr() != x0.data_ptr() and args[2] == p.data_ptr() and torch.equal(x0, keep)
    assert tuple(args[3:9]) == (16, 4, 5, 0.05, 1.5, 0.8)
    if form == "scalar":
        assert tuple(args[9:12]) == (_lib.MASS_SCALAR, 0.37, None)
    else:
        assert args[9] == _lib.MASS_DIAG and args[10] == 0.0 and args[11] == s.mass.data_ptr()
    assert tuple(args[12:]) == (1, 1, None, None, 7, 11, None)


@pytest.mark.parametrize("form", FORMS)
def test_the_fused_ghmc_route_is_one_recorded_launch(fused_cpu, monkeypatch, form):  # noqa: F811
    reserved = []
    mass = 0.37 if form == "scalar" else mc.diag_mass(4)
    s, rec = _massed(fused_cpu, monkeypatch, ta.GeneralizedHMC, mass, n_leapfrog_steps=3)
    monkeypatch.setattr(_rng, "reserve", lambda generator, device, n_steps: reserved.append(n_steps) or (7, 11))
    x0 = torch.randn(16, 4, generator=_gen(1))
    v0 = torch.ones(16, 4)
    traj, diag, p = s.sample(x=x0, n_steps=5, thin=2, velocity=v0, return_trajectory=True, return_diagnostics=True, return_velocity=True)
    assert reserved == [2 * 5 + 1] and len(rec.named(GHMC_ENTRY)) == 1 and not rec.named("ebm_ghmc_chain_f32")
    name, args = rec.calls[0]
    assert name == GHMC_ENTRY and args[2] == p.data_ptr() != v0.data_ptr() and torch.equal(v0, torch.ones(16, 4))
    assert tuple(args[3:10]) == (16, 4, 5, 3, 0.05, 1.5, 0.8)
    if form == "scalar":
        assert tuple(args[10:13]) == (_lib.MASS_SCALAR, 0.37, None)
    else:
        assert args[10] == _lib.MASS_DIAG and args[11] == 0.0 and args[12] == s.mass.data_ptr()
    assert tuple(args[13:16]) == (0, 2, traj.data_ptr()) and args[16] is not None and tuple(args[17:]) == (None, None, 7, 11, None)


@pytest.mark.parametrize("cls,entry", [(ta.UnderdampedLangevin, BAOAB_ENTRY), (ta.GeneralizedHMC, GHMC_ENTRY)])
def test_sample_moments_never_launches_the_unit_mass_moments_kernel(fused_cpu, monkeypatch, cls, entry):  # noqa: F811
    s, rec = _massed(fused_cpu, monkeypatch, cls, mc.diag_mass(4))
    x, mom, p = s.sample_moments(x=torch.randn(16, 4, generator=_gen(1)), n_steps=6, return_velocity=True)
    assert not rec.named("ebm_kinetic_moments") and len(rec.named(entry)) == 6  # step by step, the massed chain entry each time
    assert mom.chain_mean.shape == (2, 16, 4)


def test_sample_moments_keeps_p_squared_over_m():
    """The v^2 average of a massed BAOAB run is that of p^2 / m, step by step."""
    mass = torch.tensor(mc.LAW_MASS)
    s = ta.UnderdampedLangevin(mc.law_model(), step_size=mc.LAW_STEP, friction=mc.LAW_GAMMA_BAOAB, temperature=mc.LAW_TEMP, mass=mass)
    x0 = mc.law_start()[:512]
    p0 = mc.start_momentum(mass, torch.randn(512, 4, generator=_gen(3)))
    _, mom, p = s.sample_moments(x=x0, n_steps=4, velocity=p0, return_velocity=True, generator=_gen(4))
    g = _gen(4)
    x, q, seen = x0, p0, []
    for _ in range(4):
        x, q = s.sample(x=x, n_steps=1, velocity=q, return_velocity=True, reset_schedulers=False, generator=g)
        seen.append(q * q / mass)
    assert torch.equal(q, p)
    want = torch.stack(seen).double().mean(dim=(0, 1))
    assert torch.allclose(mom.kinetic_temperature, want, rtol=1e-5)
    assert not torch.allclose(mom.kinetic_temperature[2:], torch.stack(seen).double().mean(dim=(0, 1))[2:] * 4.0, rtol=0.5)  # (not p^2)


def test_diagonal_mass():
    g = _gen(5)
    sigma = torch.tensor([2.0, 0.5, 0.1])
    s = ta.GeneralizedHMC(ta.GaussianModel(torch.zeros(3), torch.diag(sigma**2)), step_size=0.05, n_leapfrog_steps=2)
    _, mom = s.sample_moments(x=sigma * torch.randn(2048, 3, generator=g), n_steps=8, generator=g)
    mass = mom.diagonal_mass()
    assert mass.dtype == torch.float32 and mass.shape == (3,) and torch.equal(mass, (1.0 / mom.var).float())
    assert torch.allclose(mass, 1.0 / sigma**2, rtol=0.1)
    # the refusal: a variance that is zero, negative or not finite
    for bad in (0.0, math.nan, math.inf):
        broken = ta.samplers.moments.ChainMoments(mom.chain_mean.clone(), mom.chain_m2.clone(), mom.half_len)
        broken._compute()["var"][1] = bad
        with pytest.raises(ValueError, match="not finite and positive"):
            broken.diagonal_mass()
    still = ta.samplers.moments.ChainMoments(torch.zeros(2, 8, 3), torch.zeros(2, 8, 3), 4)  # chains that never moved: var = 0
    with pytest.raises(ValueError, match="not finite and positive"):
        still.diagonal_mass()


# ---------------------------------------------------------------------------------
# the refusals of the two entries
# ---------------------------------------------------------------------------------
def baoab_abi_call(desc, *, x=16, v=16, n=4, dim=8, k=3, h=0.1, gamma=1.0, temp=1.0, mass_kind=_lib.MASS_SCALAR, mass=0.5, diag=None,
                   thin=1):
    _lib.call(BAOAB_ENTRY, desc, x, v, n, dim, k, h, gamma, temp, mass_kind, mass, diag, 0, thin, None, None, 0, 0, None)


def ghmc_abi_call(desc, *, x=16, v=16, n=4, dim=8, n_mh=3, L=2, eps=0.1, gamma=1.0, temp=1.0, mass_kind=_lib.MASS_SCALAR, mass=0.5,
                  diag=None, thin=1):
    _lib.call(GHMC_ENTRY, desc, x, v, n, dim, n_mh, L, eps, gamma, temp, mass_kind, mass, diag, 0, thin, None, None, None, None, 0, 0, None)


MASS_REFUSALS = [
    (dict(mass_kind=_lib.MASS_NONE), ValueError, "mass_kind=0"),
    (dict(mass_kind=3), ValueError, "mass_kind=3"),
    (dict(mass_kind=_lib.MASS_DIAG, diag=None), ValueError, "mass_diag is NULL"),
    (dict(mass=0.0), ValueError, "mass_scalar=0 "),
    (dict(mass=-2.0), ValueError, "mass_scalar=-2"),
    (dict(mass=float("inf")), ValueError, "mass_scalar=inf"),
    (dict(mass=float("nan")), ValueError, "mass_scalar=nan"),
]


def baoab_refusals():
    from test_kinetic import REFUSALS

    return REFUSALS + MASS_REFUSALS


def ghmc_refusals():
    from test_ghmc import REFUSALS

    return REFUSALS + MASS_REFUSALS


@pytest.mark.parametrize("call,refusals,what", [(baoab_abi_call, baoab_refusals, "no underdamped-Langevin kernel"),
                                                (ghmc_abi_call, ghmc_refusals, "no generalized-HMC kernel")])
def test_abi_refusals_need_no_gpu(call, refusals, what):
    """Everything the unit-mass entry refuses and the mass refusals, in front of any launch (the pointers are never dereferenced)."""
    desc = _lib.EnergyDesc()
    desc.kind = _lib.ENERGY_DOUBLE_WELL
    for kw, exc, match in refusals():
        with pytest.raises(exc, match=match):
            call(desc, **kw)
    with pytest.raises(ValueError, match="energy descriptor is NULL"):
        call(None)
    desc.kind, desc.dev0 = _lib.ENERGY_MLP, 16
    with pytest.raises(RuntimeError, match=r"code -2.*" + what):  # EBM_EKIND
        call(desc)
    desc.kind = _lib.ENERGY_DOUBLE_WELL
    call(desc, n=0)  # an empty call returns in front of any launch
    call(desc, n=0, mass_kind=_lib.MASS_DIAG, diag=16)
    with pytest.raises(ValueError, match="mass_kind=0"):  # ... but behind the mass checks
        call(desc, n=0, mass_kind=_lib.MASS_NONE)


def test_the_entries_are_exported_and_declared():
    import os
    import re

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ebm_hip.h")).read()

    def params(name):
        m = re.search(r"EBM_API\s+int\s+" + name + r"\s*\(([^)]*)\)", header)
        assert m, name
        return re.sub(r"\s+", " ", m.group(1)).strip()

    three = "int32_t mass_kind, double mass_scalar, const float* mass_diag, "
    for entry, unit in ((BAOAB_ENTRY, "ebm_kinetic_chain_f32"), (GHMC_ENTRY, "ebm_ghmc_chain_f32")):
        assert entry in _lib.EXPORTS and hasattr(_lib.lib(), entry)
        assert params(entry) == params(unit).replace("double temperature, ", "double temperature, " + three)
        proto, unit_proto = _lib._PROTOTYPES[entry][1], _lib._PROTOTYPES[unit][1]
        at = len(unit_proto) - (7 if unit == "ebm_kinetic_chain_f32" else 9)  # behind `temperature`
        assert proto == unit_proto[:at] + [_lib._i32, _lib._d, _lib._p] + unit_proto[at:]
    assert _lib.ABI_VERSION == 9 and len(_lib.EXPORTS) == 58
